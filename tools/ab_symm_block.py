#!/usr/bin/env python3
"""A/B of rmsf_symm_block (csrc/eigen_block.hip, Y = M Q) between builds of
the library with other plan and pipeline constants, in one process.

The builds come from tools/build_ab.sh, which passes -D flags to the Makefile;
the constants are the RMSF_SYMM_* macros at the top of csrc/eigen_block.hip:

    tools/build_ab.sh tg768  -DRMSF_SYMM_TARGET_GROUPS=768
    tools/build_ab.sh tg2048 -DRMSF_SYMM_TARGET_GROUPS=2048
    tools/build_ab.sh lb4    -DRMSF_SYMM_WAVES_PER_SIMD=4
    tools/build_ab.sh ku4    -DRMSF_SYMM_KSTEPS=4
    tools/build_ab.sh lb4ku1 -DRMSF_SYMM_WAVES_PER_SIMD=4 -DRMSF_SYMM_KSTEPS=1
    python tools/ab_symm_block.py [--out profiles/pca_eig_symm_variants.json]

Every tools/_ab/librmsf_*.so and the in-tree library (``tree``) are timed at
642^2 and 10,023^2 with 16, 32 and 48 columns: device events around
``--inner`` back-to-back calls through ctypes, two warm-up rounds, median of
``--reps``; each result is compared with torch's ``M @ Q``.  ``ranges`` is
the number of k-ranges the build's plan cuts the contraction into.

The in-tree library is also timed through ``Engine.symm_block``
(``tree_engine``), the call tools/bench_pca_eig.py times.  At 642^2 the two
launches of a call take less device time than the host needs to issue them, so
both figures there are issue rates -- of the bare ctypes call and of the
wrapper with its argument checks -- and do not compare kernels; the variants
are told apart at 10,023^2.
"""
import argparse
import ctypes
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

SIZES = (642, 10_023)
COLS = (16, 32, 48)


def timed(fn, reps, inner):
    import torch
    ms = []
    for i in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_eig_symm_variants.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args(argv)

    import torch

    from rmsf_amd._lib import LIB_PATH, SIGNATURES
    from rmsf_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("ab_symm_block needs a HIP device")
    eng = Engine(torch.device("cuda", 0))
    libs = {"tree": LIB_PATH}
    for path in sorted(glob.glob(os.path.join(ROOT, "tools", "_ab", "librmsf_*.so"))):
        libs[os.path.basename(path)[len("librmsf_"):-len(".so")]] = path
    data = {}
    for n in SIZES:
        g = torch.Generator(device="cuda").manual_seed(n)
        m = torch.randn(n, n, device="cuda", dtype=torch.float64, generator=g)
        data[n] = ((m + m.T).contiguous(), torch.randn(n, 48, device="cuda", dtype=torch.float64, generator=g))
    out = {"device": torch.cuda.get_device_name(0), "inner_calls": a.inner, "reps": a.reps, "builds": {}}
    st = torch.cuda.current_stream().cuda_stream
    for name, path in libs.items():
        lib = ctypes.CDLL(path)
        if not hasattr(lib, "rmsf_symm_block"):   # a build from before the kernel
            continue
        for f in ("rmsf_symm_block", "rmsf_symm_block_workspace_bytes"):
            getattr(lib, f).restype, getattr(lib, f).argtypes = SIGNATURES[f]
        entry = {}
        for n in SIZES:
            m, q = data[n]
            for cols in COLS:
                y = torch.zeros(n, cols, device="cuda", dtype=torch.float64)
                need = lib.rmsf_symm_block_workspace_bytes(n, cols)
                work = torch.empty(max(1, need // 8), device="cuda", dtype=torch.float64)

                def call():
                    rc = lib.rmsf_symm_block(m.data_ptr(), n, n, q.data_ptr(), 48, cols, y.data_ptr(), cols,
                                             work.data_ptr(), need, st)
                    assert rc == 0, rc

                ms = timed(call, a.reps, a.inner)
                ref = m @ q[:, :cols]
                err = float((y - ref).abs().max() / ref.abs().max())
                assert err < 1e-12, (name, n, cols, err)
                entry[f"n{n}_cols{cols}"] = {"ms": ms, "ranges": max(1, need // (8 * n * cols))}
                print(name, n, cols, json.dumps(entry[f"n{n}_cols{cols}"]), flush=True)
        out["builds"][name] = entry
    entry = {}
    for n in SIZES:
        m, q = data[n]
        for cols in COLS:
            y = eng.empty(n, cols)
            need = eng.symm_block_workspace_bytes(n, cols)
            work = eng.empty(need // 8) if need else None
            ms = timed(lambda: eng.symm_block(m, n, q, cols, y, work), a.reps, a.inner)
            entry[f"n{n}_cols{cols}"] = {"ms": ms}
            print("tree_engine", n, cols, json.dumps(entry[f"n{n}_cols{cols}"]), flush=True)
    out["tree_engine"] = entry
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
