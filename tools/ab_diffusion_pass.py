#!/usr/bin/env python
"""rmsf_diffusion_kernel (csrc/diffusion.hip) with other waves-per-row and
loads-in-flight constants, all in one process on one matrix: device-event ms
per call, the variants alternating repetition by repetition after two warm-up
rounds, and the bytes per second of the 8 F^2 bytes read and 8 F^2 written.
The distances are restored before every call, outside the timed span.

The variants are builds of the library beside the in-tree one:

    tools/build_ab.sh diff_w8u4 -DRMSF_DIFF_WAVES=8 -DRMSF_DIFF_UNROLL=4
    python tools/ab_diffusion_pass.py --variants diff_w8u4,... [--frames 4096,20000] [--out FILE.json]

``tree`` is the in-tree library.  The kernel values of every variant are
compared with the tree's in their bits (the transform is element-wise: they
must be equal); the row sums, whose order follows the constants, within
F 2^-52 relative.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread  # noqa: E402  (beside this file)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variants", default="")
    ap.add_argument("--frames", default="4096,20000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--epsilon", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    import torch

    from rmsf_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("ab_diffusion_pass needs a HIP device; nothing is measured without one")
    libs = {"tree": _lib.load()}
    for name in [v for v in a.variants.split(",") if v]:
        libs[name] = _lib.load(os.path.join(ROOT, "tools", "_ab", f"librmsf_{name}.so"))
    stream = torch.cuda.current_stream().cuda_stream
    result = {"device": torch.cuda.get_device_name(0), "epsilon": a.epsilon, "shapes": {}}
    for n in [int(s) for s in a.frames.split(",") if s]:
        d = torch.rand((n, n), dtype=torch.float64, device="cuda:0") * 3.0
        work = torch.empty_like(d)
        rowsum = {k: torch.empty(n, dtype=torch.float64, device="cuda:0") for k in libs}
        ms = {k: [] for k in libs}
        same = {}
        ref = None
        for i in range(a.reps + 2):
            for k, lib in libs.items():
                work.copy_(d)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = lib.rmsf_diffusion_kernel(work.data_ptr(), n, n, a.epsilon, rowsum[k].data_ptr(), stream)
                e1.record()
                torch.cuda.synchronize()
                assert rc == 0, (k, rc)
                if i >= 2:
                    ms[k].append(e0.elapsed_time(e1))
                if i == 0:
                    if k == "tree":
                        ref = work.clone()
                    same[k] = bool(torch.equal(work, ref)) and bool(
                        ((rowsum[k] - rowsum["tree"]).abs() <= n * 2.0 ** -52 * rowsum["tree"]).all())
        del ref
        entry = {}
        for k in libs:
            entry[k] = dict(spread(ms[k]), tbs=16 * n * n / (statistics.median(ms[k]) * 1e-3) / 1e12,
                            same_as_tree=same[k])
        result["shapes"][str(n)] = entry
        print(n, json.dumps(entry), flush=True)
        del d, work, rowsum
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
