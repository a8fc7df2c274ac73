#!/usr/bin/env python3
"""Cycles of a pass of the urn chain by section, one region of the configs[1] shape (a launch per level).

Needs the experiment build of the library (`make -C rambl_amd/csrc clean && make -C rambl_amd/csrc EXTRA=-DSC_CHAIN_PROF`),
which stamps the shader clock on wavefront 0 between the sections of every pass (sc_sampler.hpp, CHAIN_STAMP) and exports
`sc_debug_chain_prof`.  A stamp costs about 50 cycles, which stay in the section in front of it.  The three stamps inside
the commit section wait for the LDS operations in front of them, so what the product build leaves in flight (the next
rows' LDS reads, the count's atomic) is charged to its own part here.

    python3 tools/chain_prof.py [regions]        (default 2: the second one runs on warm buffers)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SECTIONS = [(0, "counts and chains"), (1, "joins and test"), (2, "first barrier and advance"),
            (3, "commit: bookkeeping (ro, upos, uniform refill)"), (6, "commit: issue_loads"),
            (7, "commit: s_kf add"), (8, "commit: symbol count / draw log"), (4, "second barrier")]


def main():
    import inflight_probe as ip
    from rambl_amd import capi, stage5
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    if not hasattr(capi.lib(), "sc_debug_chain_prof"):
        sys.exit("this library was built without -DSC_CHAIN_PROF")
    base = ip.prepare(1, 10000)
    ctx = capi.Context(0, 1)
    params = capi.default_params(0.01, 0.02, 0.02)
    stage5.run_regions(ctx, base * n, 1, params)
    out = (ctypes.c_ulonglong * 12)()
    rc = capi.lib().sc_debug_chain_prof(out)
    ctx.close()
    if rc != 0:
        sys.exit("sc_debug_chain_prof: hip error %d" % rc)
    v = list(out)
    passes = max(v[5], 1)
    print("passes %d" % v[5])
    print("| section of the pass | cycles |")
    print("|---|---|")
    for i, name in SECTIONS:
        print("| %s | %.1f |" % (name, v[i] / passes))
    print("| sum | %.1f |" % (sum(v[i] for i, _ in SECTIONS) / passes))


if __name__ == "__main__":
    main()
