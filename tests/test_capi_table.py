"""CPU: the binding's one prototype table (capi.ENTRIES), its Structure mirrors and its error constants against
include/straincall_hip.h as a whole -- every declaration type by type, every struct member by member.  The header is parsed
here and only here; the library is loaded but no compute call is made."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "straincall_hip.h")
RETURNS = {"int": C.c_int, "void": None, "long": C.c_long, "double": C.c_double, "const char*": C.c_char_p}
SCALARS = {"int": C.c_int, "long": C.c_long, "double": C.c_double, "unsigned long long": C.c_ulonglong}
POINTEES = dict(SCALARS, **{"unsigned": C.c_uint, "unsigned char": C.c_ubyte})
N_DECLARED = 53         # the functions the header declares today (the library exports one more, sc_add_ones, which is no part of the ABI)


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def complete_structs(hdr):
    """{struct name: body text} of every struct the header defines, in its order."""
    return dict(re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", hdr, flags=re.S))


def opaque_structs(hdr):
    return set(re.findall(r"typedef struct (\w+) \1;", hdr))


def mirror(struct):
    """sc_profile_count_stats -> capi.ScProfileCountStats."""
    from rambl_amd import capi
    return getattr(capi, "".join(w.capitalize() for w in struct.split("_")))


def declarations(hdr):
    """[(return type, name, [parameter type texts])]: names dropped, const dropped, `T* *` written as T**."""
    body = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", hdr, flags=re.S)
    out = []
    for ret, name, params in re.findall(r"^(const char\*|int|void|long|double)\s+(sc_\w+)\s*\(([^)]*)\)\s*;", body, flags=re.M):
        types = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            t = re.sub(r"\bconst\b", "", re.sub(r"\w+\s*$", "", p.strip()))          # the parameter's name is its last word
            types.append(re.sub(r"\s*\*\s*", "*", " ".join(t.split())))
        out.append((ret, name, types))
    return out


def bound_type(text, complete, opaque):
    """The ctypes type a parameter written `text` must be bound to."""
    base, stars = text.rstrip("*"), len(text) - len(text.rstrip("*"))
    assert "*" not in base, text
    if stars == 0:
        return SCALARS[base]
    if stars == 1:
        if base == "char":
            return C.c_char_p
        if base in POINTEES:
            return C.POINTER(POINTEES[base])
        if base in complete:
            return C.POINTER(mirror(base))
        assert base in opaque, text
        return C.c_void_p
    assert stars == 2, text
    return C.POINTER(bound_type(base + "*", complete, opaque))          # a pointer to a pointer: a pointer to what the inner one binds to


def test_every_declaration_is_a_row_of_the_table_type_by_type():
    from rambl_amd import capi
    hdr = header_text()
    complete, opaque = complete_structs(hdr), opaque_structs(hdr)
    decls = declarations(hdr)
    names = [name for _, name, _ in decls]
    assert names == re.findall(r"\b(sc_\w+)\s*\(", hdr)          # the structured pattern misses no call-like text of the header
    assert len(names) >= N_DECLARED and len(set(names)) == len(names)
    assert capi.EXPORTS == names and len(capi.ENTRIES) == len(names)          # one row each, in the header's order
    rows = {name: (restype, argtypes) for name, restype, argtypes in capi.ENTRIES}
    lib = capi.lib()
    for ret, name, params in decls:
        restype, argtypes = rows[name]
        assert restype is RETURNS[ret], name
        assert len(argtypes) == len(params), name
        for k, text in enumerate(params):
            assert argtypes[k] is bound_type(text, complete, opaque), "%s: argument %d (%s) is bound to %s" % (name, k, text, argtypes[k])
        f = getattr(lib, name)                                   # and the loaded library carries the row
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    assert not hasattr(capi, "sc_debug_chain_prof") and "sc_debug_chain_prof" not in rows


def members(body, complete, prefix=""):
    """[(member path as C writes it, name on the flat ctypes side)] of a struct body, nested complete structs flattened."""
    out = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.match(r"((?:unsigned |long )*\w+) (.*)$", stmt)
        assert m, stmt
        for decl in m.group(2).split(","):
            name = re.match(r"\s*(\w+)\s*(\[\d+\])?\s*$", decl)
            assert name, stmt
            if m.group(1) in complete:
                out += members(complete[m.group(1)], complete, prefix + name.group(1) + ".")
            else:
                out.append((prefix + name.group(1), name.group(1)))
    return out


def test_every_struct_layout_matches_its_mirror(tmp_path):
    hdr = header_text()
    complete = complete_structs(hdr)
    assert list(complete) == ["sc_params", "sc_stats", "sc_depth_stats", "sc_align_stats", "sc_profile_stats", "sc_profile_seed_stats",
                              "sc_profile_count_stats", "sc_profile_cohort_stats", "sc_taxa_stats"]
    listed = {s: members(body, complete) for s, body in complete.items()}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "straincall_hip.h"', 'int main(void) {']
    for s, ms in listed.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for path, _ in ms:
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, path, s, path, s, path))
    lines += ['    return 0;', '}', '']
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-std=gnu11", "-Wall", "-I", os.path.dirname(HEADER), "-o", exe, src])
    printed = {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        key, *numbers = line.split()
        printed[key] = tuple(int(x) for x in numbers)
    for s, ms in listed.items():
        m = mirror(s)
        assert issubclass(m, C.Structure), s
        assert [flat for _, flat in ms] == [f for f, _ in m._fields_], s          # names and order
        assert C.sizeof(m) == printed[s][0], "%s: sizeof %d in C, %d in ctypes" % (s, printed[s][0], C.sizeof(m))
        for path, flat in ms:
            field = getattr(m, flat)
            assert (field.offset, field.size) == printed["%s.%s" % (s, path)], "%s.%s: (offset, size) %s in C, (%d, %d) in ctypes" % (
                s, path, printed["%s.%s" % (s, path)], field.offset, field.size)
    assert len(listed["sc_stats"]) == 28 and printed["sc_stats.kind_levels"][0] == 288 and printed["sc_profile_cohort_stats.n_allocs"][0] == 160


def test_statistics_share_one_as_dict():
    """Array members come out as lists by their type, everything else as the value; one definition for every statistics struct."""
    from rambl_amd import capi, stage1
    assert stage1.DepthStats is capi.ScDepthStats
    for s in complete_structs(header_text()):
        m = mirror(s)
        if s == "sc_params":
            continue
        assert issubclass(m, capi.Stats) and "as_dict" not in vars(m), s
        d = m().as_dict()
        assert list(d) == [f for f, _ in m._fields_]
        for f, t in m._fields_:
            assert (type(d[f]) is list and len(d[f]) == t._length_) if issubclass(t, C.Array) else d[f] == 0, (s, f)
    st = capi.ScStats()
    st.kind_levels[16], st.host_us[2] = 7, 0.5
    d = st.as_dict()
    assert d["kind_levels"] == [0] * 16 + [7] and d["host_us"] == [0.0, 0.0, 0.5] and d["xcd_levels"] == [0] * 8 and d["wake_us"] == [0.0, 0.0]


def test_error_constants_are_the_headers():
    from rambl_amd import capi
    defined = {k: int(v) for k, v in re.findall(r"#define (SC_OK|SC_ERR_\w+) \(?(-?\d+)\)?", header_text())}
    assert len(defined) == 7 and defined["SC_OK"] == 0
    for name, value in defined.items():
        assert getattr(capi, name) == value, name
    assert capi.ERRORS == {v: k for k, v in defined.items() if k != "SC_OK"}
    assert capi.StrainCallError(defined["SC_ERR_CAPACITY"]).code == capi.SC_ERR_CAPACITY
    assert str(capi.StrainCallError(capi.SC_ERR_ARG, "x")) == "SC_ERR_ARG (-3): x"


def test_with_room_grows_to_the_reported_number_only():
    """The one growth loop: it repeats at the reported number while the answer is SC_ERR_CAPACITY with more than there was
    room for, and hands every other answer back as it is."""
    from rambl_amd import capi
    seen = []

    def attempt(cap, answers={4: (capi.SC_ERR_CAPACITY, 9), 9: (capi.SC_ERR_CAPACITY, 30), 30: (capi.SC_OK, 30)}):
        seen.append(cap)
        return answers[cap] + ("kept at %d" % cap,)
    assert capi.with_room(4, attempt) == (capi.SC_OK, 30, "kept at 30") and seen == [4, 9, 30]
    for answer in ((capi.SC_ERR_CAPACITY, 4), (capi.SC_ERR_CAPACITY, 0), (capi.SC_ERR_ARG, 99), (capi.SC_OK, 2)):
        calls = []
        assert capi.with_room(4, lambda cap: calls.append(cap) or answer + (None,)) == answer + (None,) and calls == [4]


def test_one_owner_frees_every_handle():
    from rambl_amd import capi
    for cls, free in ((capi.NativeAln, "sc_aln_close"), (capi.NativeReads, "sc_reads_free"), (capi.ProfileIndex, "sc_profile_index_free"),
                      (capi.TaxaModel, "sc_taxa_free")):
        assert issubclass(cls, capi.Handle) and cls._free == free and free in capi.EXPORTS
        assert not {"close", "__del__", "__enter__", "__exit__"} & set(vars(cls)), cls
        h = cls.__new__(cls)
        h.close()                                                # nothing was opened: nothing to free, and no call
        with h as same:
            assert same is h and not h._h
