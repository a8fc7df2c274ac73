"""CPU: the C-ABI library loads and exports every symbol include/*.h declares
(no compute call is made without a GPU), and the Python binding refuses to run
without a device instead of falling back."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    names = []
    inc = os.path.join(ROOT, "include")
    for f in os.listdir(inc):
        if f.endswith(".h"):
            txt = open(os.path.join(inc, f)).read()
            txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
            names += re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", txt)
    return sorted(set(names))


def test_library_exports_header_symbols():
    from rambl_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 53 and "sc_profile_evalue6" in names and "sc_update_level" in names and "sc_hard_level" in names
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(capi.EXPORTS) == names


def test_no_cpu_fallback():
    import torch
    from rambl_amd import capi
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(capi.StrainCallError) as e:
        capi.Context(0, 1)
    assert e.value.code == -1


def test_product_never_touches_oracle():
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "rambl_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                if re.search(r"oracle/|liboracle|straincall_oracle|import\s+oracle", txt):
                    bad.append(os.path.join(dirpath, f))
    assert bad == []


def test_graph_stage_test_entries_are_declared_and_bound():
    """sc_roi_thread_edges and sc_edge_support_tables (test entries): in the header, exported, bound with as many arguments
    as the header declares; sc_roi_thread_tables keeps its ten."""
    from rambl_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "straincall_hip.h")).read(), flags=re.S)
    lib = capi.load_library()
    for name, n_args in (("sc_roi_thread_edges", 7), ("sc_edge_support_tables", 11), ("sc_roi_thread_tables", 10)):
        decl = re.search(r"\bint %s\s*\(([^)]*)\)" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert name in capi.EXPORTS
        f = getattr(lib, name)
        assert len(f.argtypes) == n_args and f.restype is ctypes.c_int, name
    assert hasattr(capi.Context, "thread_edges") and hasattr(capi.Context, "edge_support_tables")
