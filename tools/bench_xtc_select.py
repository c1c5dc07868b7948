"""Selected against whole-frame GPU XTC decode at RMSF.py's own ratio (not
product code): 47,681 atoms, a 214-atom selection (RMSF.py:34,77,126).

Writes a synthetic XTC (a protein-like chain first, then 3-atom waters, as a
GRO lists them; the selection is every 15th atom of the chain, where CA atoms
sit) and times, with >= 5 repeats each (min and median):

  (a) the decode kernel alone, whole frames against the selected atoms, by
      events around the launches (records resident in HBM);
  (b) one sweep, align=None, through XtcSource;
  (c) RMSF.py's two sweeps, align="average", cache=True.

For (b) and (c) it reports the HBM bytes of the decoder's frame slots plus the
cache (from the sizes, and as the drop in free device memory) and whether the
cache was granted.  The selected path's slots + cache are n_sel/n_atoms of the
whole-frame path's, plus the map: asserted.

    python tools/bench_xtc_select.py [--frames N] [--repeats R] [--out FILE]
    python tools/bench_xtc_select.py --baseline-only     # a tree without the feature
    python tools/bench_xtc_select.py --compare BASE.json # verdict against such a run

--baseline-only uses nothing but the API a tree without selected decode has
(XtcSource without decode_select, rmsf_xtc_decode_records): run it in the
parent commit's tree, on the same device in the same visit, for the baseline.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_ATOMS, N_SEL, N_CHAIN = 47_681, 214, 3_341
KERNEL_FRAMES = 2048  # frames per timed launch of (a): 8 waves per CU, throughput not latency


def selection():
    return (5 + 15 * np.arange(N_SEL)).astype(np.int64)  # inside the chain: 5 .. 3200


def write_file(path, n_frames, chunk=100):
    """Chain + waters, drifting per frame (the shape of tests' _protein_like);
    returns the seconds the writing took."""
    from rmsf_amd.xtc import write_xtc
    rng = np.random.default_rng(47681)
    base = np.empty((N_ATOMS, 3))
    base[:N_CHAIN] = np.cumsum(rng.normal(0, 1.5, (N_CHAIN, 3)), axis=0) + 40.0
    n_w = (N_ATOMS - N_CHAIN) // 3
    base[N_CHAIN:N_CHAIN + 3 * n_w] = (np.repeat(rng.uniform(0, 80, (n_w, 3)), 3, axis=0)
                                       + rng.normal(0, 0.9, (3 * n_w, 3)))
    base[N_CHAIN + 3 * n_w:] = rng.uniform(0, 80, (N_ATOMS - N_CHAIN - 3 * n_w, 3))
    base = base.astype(np.float32)
    t0 = time.perf_counter()
    for f in range(0, n_frames, chunk):
        n = min(chunk, n_frames - f)
        x = base[None] + rng.standard_normal((n, N_ATOMS, 3), dtype=np.float32) * np.float32(0.3)
        write_xtc(path, x, append=f > 0)
    return time.perf_counter() - t0


def stats(ts):
    return {"min_ms": 1e3 * min(ts), "median_ms": 1e3 * statistics.median(ts), "max_ms": 1e3 * max(ts),
            "repeats": len(ts)}


def kernel_alone(path, sel, repeats, baseline_only):
    """(a): KERNEL_FRAMES records in HBM, events around the launch."""
    from rmsf_amd._lib import call
    from rmsf_amd.xtc import XTCFile
    with XTCFile(path) as f:
        n = min(KERNEL_FRAMES, f.n_frames)
        rec = [f.record(i) for i in range(n)]
    words = np.fromfile(path, dtype=np.uint32, count=(rec[-1][0] + rec[-1][1]) // 4)
    dev = torch.device("cuda")
    d_words = torch.as_tensor(words.view(np.int32)).to(dev)
    d_off = torch.as_tensor(np.array([o // 4 for o, _ in rec], dtype=np.int64)).to(dev)
    d_len = torch.as_tensor(np.array([b // 4 for _, b in rec], dtype=np.int64)).to(dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    out = {"frames": n}

    def timed(launch):
        ts = []
        for r in range(repeats + 2):  # two warm-up launches
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            if r >= 2:
                ts.append(e0.elapsed_time(e1) * 1e-3)
        assert int(st.abs().sum()) == 0
        return stats(ts)

    full = torch.empty((n, N_ATOMS, 3), dtype=torch.float32, device=dev)
    out["whole_frames"] = timed(lambda: call("rmsf_xtc_decode_records", d_words.data_ptr(), d_off.data_ptr(),
                                             d_len.data_ptr(), n, N_ATOMS, full.data_ptr(), 3 * N_ATOMS,
                                             st.data_ptr(), s))
    if not baseline_only:
        m = np.full(N_ATOMS, -1, dtype=np.int32)
        m[sel] = np.arange(len(sel), dtype=np.int32)
        d_map = torch.as_tensor(m).to(dev)
        part = torch.empty((n, len(sel), 3), dtype=torch.float32, device=dev)
        out["selected"] = timed(lambda: call("rmsf_xtc_decode_records_sel", d_words.data_ptr(), d_off.data_ptr(),
                                             d_len.data_ptr(), n, N_ATOMS, d_map.data_ptr(), len(sel),
                                             part.data_ptr(), 3 * len(sel), st.data_ptr(), s))
        assert torch.equal(part, full[:, torch.as_tensor(sel).to(dev)])
    return out


def sweeps(path, sel, repeats, align, cache, kw):
    """(b) / (c): RMSF(...).run() over a fresh source per repeat."""
    from rmsf_amd import RMSF
    from rmsf_amd.sources import XtcSource
    ts, info, rmsf = [], None, None
    for r in range(repeats + 1):  # one warm-up run
        torch.cuda.synchronize()
        torch.cuda.empty_cache()  # the previous repeat's cache back to the device: the drop below counts it
        free0 = torch.cuda.mem_get_info()[0]
        src = XtcSource(path, sel, cache=cache, **kw)
        t0 = time.perf_counter()
        rmsf = RMSF(src, align=align).run().results.rmsf
        dt = time.perf_counter() - t0
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        if r >= 1:
            ts.append(dt)
        rows = src.n_sel if getattr(src, "decode_select", False) else src.n_atoms
        granted = src.cache is not None
        # with a cache the decoder writes into it (no slot frame buffers)
        slots = 0 if granted else src.decoder.n_slots * src.batch_frames * rows * 12
        info = {"rows_per_frame": rows, "batch_frames": src.batch_frames, "cache_asked": cache,
                "cache_granted": granted, "slot_frame_bytes": slots,
                "cache_bytes": src.n_traj * rows * 12 if granted else 0,
                "map_bytes": 4 * src.n_atoms if rows != src.n_atoms else 0,
                "free_memory_drop_bytes": free0 - free1}
        info["hbm_slots_plus_cache_bytes"] = info["slot_frame_bytes"] + info["cache_bytes"] + info["map_bytes"]
        src.decoder.close()
        del src
    return {**stats(ts), **info}, rmsf


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the synthetic file goes (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--compare", default=None, help="a --baseline-only JSON: add the not-slower verdicts")
    a = ap.parse_args()
    assert a.repeats >= 5, "at least 5 repeats"
    d = a.dir or tempfile.mkdtemp(prefix="xtc_select_")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, f"sel_{N_ATOMS}x{a.frames}.xtc")
    res = {"n_atoms": N_ATOMS, "n_sel": N_SEL, "n_frames": a.frames, "baseline_only": a.baseline_only,
           "device": torch.cuda.get_device_name(0)}
    res["write_seconds"] = write_file(path, a.frames)
    res["file_bytes"] = os.path.getsize(path)
    sel = selection()
    res["a_kernel_alone"] = kernel_alone(path, sel, a.repeats, a.baseline_only)
    legs = {"default": {}} if a.baseline_only else {"decode_select": {"decode_select": True},
                                                    "whole_frames": {"decode_select": False}}
    ref = None
    for name, kw in legs.items():
        b, r1 = sweeps(path, sel, a.repeats, None, False, kw)
        c, r2 = sweeps(path, sel, a.repeats, "average", True, kw)
        res[name] = {"b_one_sweep": b, "c_two_sweeps_cached": c}
        if ref is None:
            ref = (r1, r2)
        else:  # the legs compute the same RMSF (other batches' rounding apart)
            assert np.abs(r1 - ref[0]).max() < 1e-9 and np.abs(r2 - ref[1]).max() < 1e-9
    if not a.baseline_only:
        # memory: the selected slots + cache are n_sel/n_atoms of the whole frames', plus the map
        for k in ("b_one_sweep", "c_two_sweeps_cached"):
            s_, w_ = res["decode_select"][k], res["whole_frames"][k]
            if s_["cache_granted"] == w_["cache_granted"]:
                assert (s_["hbm_slots_plus_cache_bytes"] - s_["map_bytes"]) * N_ATOMS \
                    == w_["hbm_slots_plus_cache_bytes"] * N_SEL, k
    if a.compare:
        base = json.load(open(a.compare))
        res["baseline"] = base
        verdict = {}
        for k in ("b_one_sweep", "c_two_sweeps_cached"):
            p, n = base["default"][k], res["decode_select"][k]
            margin = p["max_ms"] - p["min_ms"]  # the parent's own run-to-run spread
            verdict[k] = {"parent_median_ms": p["median_ms"], "selected_median_ms": n["median_ms"],
                          "margin_ms": margin, "not_slower": n["median_ms"] <= p["median_ms"] + margin,
                          "hbm_ratio": n["hbm_slots_plus_cache_bytes"] / max(1, p["hbm_slots_plus_cache_bytes"])}
        res["verdict"] = verdict
    os.remove(path)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
