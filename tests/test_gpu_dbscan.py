"""GPU tier of DBSCAN (csrc/dbscan.hip): the component rounds, the cluster ids
and the border rows on ``Engine.adjacency_pack``'s bits, and ``DBSCAN`` end to
end, against the numpy restatement of the definition in
tests/test_dbscan_host.py and against ``rmsf_cluster_dbscan_host``.

Everything after the threshold is integers: labels and core rows are compared
for equality, and no tolerance appears anywhere.  Where a trajectory is
clustered, the reference runs on ``DistanceMatrix``'s own matrix of the same
input -- the same kernel on the same inputs, reproducible bit for bit, so no
threshold can flip; the matrix kernel is not under test here."""
import functools

import numpy as np
import pytest

from test_clustering_host import nan_case
from test_dbscan_host import (CHAIN_M, TOUCHING, assert_consequences, assert_nan_frame, assert_same, core_rows_of,
                              dbscan_reference, host_dbscan, matrix, reference)
from test_gpu_clustering import N_FRAMES, N_STATES, RADIUS, TRAJ_CASES, traj_kw

pytestmark = pytest.mark.gpu

POISON = 2 ** 64 - 1
SIZES = [1, 63, 64, 65, 130, 1000]


def device_dbscan(d, eps, m):
    """Engine.adjacency_pack + Engine.cluster_dbscan -> (labels int64, core rows int64, n_clusters, n_rounds)."""
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    n = d.shape[0]
    adj, count = eng.adjacency_pack(torch.tensor(d, device="cuda:0"), eps)
    adj_before, count_before = adj.clone(), count.clone()
    label, core, k, rounds = eng.cluster_dbscan(adj, count, m)
    assert label.dtype == torch.int32 and label.shape == (n,) and core.shape == ((n + 63) // 64,)
    first = (label.cpu().numpy(), core.cpu().numpy())
    label2, core2, k2, rounds2 = eng.cluster_dbscan(adj, count, m)
    for a, b in zip(first, (label2.cpu().numpy(), core2.cpu().numpy())):
        assert a.tobytes() == b.tobytes()                                     # a second run: the same bytes
    assert (k2, rounds2) == (k, rounds)
    assert torch.equal(count, count_before) and torch.equal(adj, adj_before)  # read, not changed
    if n % 64:
        assert not int(first[1].view(np.uint64)[-1]) >> (n % 64)              # core bits at or past n are zero
    return first[0].astype(np.int64), core_rows_of(first[1], n), k, rounds


LOOP_CASES = ([(kind, n, m) for kind in ("points", "lattice") for n in SIZES for m in (1, 4)]
              + [("points", 4097, 4)]
              + [(kind, n, CHAIN_M) for kind in ("chain", "chain_shuffled") for n in (130, 1000)]
              + [("touching", n, TOUCHING[n][1]) for n in TOUCHING]
              + [("zero", 130, 1), ("zero", 130, 2), ("inf", 130, 1), ("inf", 130, 8), ("nan", 130, 1), ("nan", 130, 2)])


@pytest.mark.parametrize("kind,n,m", LOOP_CASES)
def test_loop(kind, n, m):
    d, eps = matrix(kind, n)
    ref = reference(kind, n, m)
    labels, core_rows, k, rounds = device_dbscan(d, eps, m)
    got = (labels, core_rows, k)
    assert_same(got, ref)
    assert_same(got, host_dbscan(d, eps, m))
    assert_consequences(d, eps, m, *got)
    assert 1 <= rounds <= ref[3], (rounds, ref[3])                            # never more rounds than plain propagation
    if kind == "points" and n == 4097:
        assert k > 1 and (labels < 0).any() and len(core_rows) < (labels >= 0).sum()   # clusters, noise and border rows
    if kind.startswith("chain"):
        assert k == 1 and len(core_rows) == n - 2 and not labels.any()        # one cluster and two border ends
    if kind == "chain_shuffled" and n == 1000:
        # plain propagation walks the path (756 rounds); hooking with shortcutting halves the trees' depth a round
        assert ref[3] == 756 and 8 * rounds <= ref[3], rounds
    if kind == "zero":
        assert (labels == -1).all() if m >= 2 else np.array_equal(labels, np.arange(n))
    if kind == "inf":
        assert k == 1 and not labels.any() and len(core_rows) == n
    if kind == "nan":
        _, small, q, keep = nan_case(n)
        assert_nan_frame(*got, dbscan_reference(small, eps, m), q, keep, m)


def test_wide_rows_keep_their_poison():
    """ldw > the words of a row: the words past them are neither read nor written."""
    import ctypes

    import torch

    from rmsf_amd import _lib
    n, m, ldw = 130, 4, 5                                                     # 3 words needed
    d, eps = matrix("points", n)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    adj = torch.full((n, ldw), -1, dtype=torch.int64, device="cuda:0")        # all-ones words
    count = torch.empty(n, dtype=torch.int32, device="cuda:0")
    _lib.call("rmsf_adjacency_pack", torch.tensor(d, device="cuda:0").data_ptr(), n, n, float(eps), adj.data_ptr(),
              ldw, count.data_ptr(), stream)
    before = adj.clone()
    label = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    core = torch.full((4,), -1, dtype=torch.int64, device="cuda:0")           # one word more than the 3 written
    need = lib.rmsf_cluster_dbscan_workspace_bytes(n)
    work = torch.empty(need // 8, dtype=torch.int64, device="cuda:0")
    k, rounds = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _lib.call("rmsf_cluster_dbscan", adj.data_ptr(), n, ldw, count.data_ptr(), m, label.data_ptr(), core.data_ptr(),
              ctypes.byref(k), ctypes.byref(rounds), work.data_ptr(), need, stream)
    torch.cuda.synchronize()
    assert torch.equal(adj, before) and bool((adj[:, 3:] == -1).all())
    words = core.cpu().numpy().view(np.uint64)
    assert words[3] == np.uint64(POISON)
    assert_same((label.cpu().numpy().astype(np.int64), core_rows_of(words[:3], n), k.value), reference("points", n, m))


# ---- past one pass of the id scan ------------------------------------------------------
BAND_N = 65_600                                                               # 1,025 words a row, about 540 MB of them


def band_words(n, cut_every_third):
    """The bit rows of the band graph i-1, i, i+1 built in HBM, no f64 matrix;
    ``cut_every_third``: the link i <-> i+1 is missing wherever (i + 1) % 3 == 0."""
    import torch
    dev = torch.device("cuda", 0)
    adj = torch.zeros((n, (n + 63) // 64), dtype=torch.int64, device=dev)
    i = torch.arange(n, device=dev)
    for delta in (-1, 0, 1):
        col = i + delta
        ok = (col >= 0) & (col < n)
        if cut_every_third and delta:
            ok &= (torch.maximum(i, col) % 3) != 0
        r, c = i[ok], col[ok]
        adj[r, c >> 6] |= torch.ones_like(c) << (c & 63)                      # (one column a row: no index repeats)
    return adj


@pytest.mark.parametrize("cut,m", [(True, 1), (False, 3)])
def test_band_graph_past_one_scan_pass(cut, m):
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    n = BAND_N
    adj = band_words(n, cut)
    count = eng.adjacency_count(adj)
    label, core, k, rounds = eng.cluster_dbscan(adj, count, m)
    labels = label.cpu().numpy().astype(np.int64)
    core_rows = core_rows_of(core.cpu().numpy(), n)
    if cut:                                                                   # runs of three, each a cluster
        assert k == 21_867 and np.array_equal(labels, np.arange(n) // 3)      # more ids than one scan pass holds words
        assert np.array_equal(core_rows, np.arange(n)) and rounds <= 3
    else:                                                                     # one path; its two ends are border rows
        assert k == 1 and not labels.any() and np.array_equal(core_rows, np.arange(1, n - 1))
        assert rounds <= 64                                                   # the path is 65,598 long


# ---- DBSCAN, end to end ------------------------------------------------------------------
EPS, MIN_SAMPLES = RADIUS, 5


@functools.lru_cache(maxsize=None)
def traj_matrix(name):
    """DistanceMatrix's own matrix of a trajectory case of tests/test_gpu_clustering.py; read-only."""
    import torch

    from rmsf_amd import DistanceMatrix
    x, _, kw = traj_kw(name)
    d = DistanceMatrix(torch.tensor(x, device="cuda:0"), **kw).run().results.dist_matrix
    d.setflags(write=False)
    return d


def first_appearance_rank(state):
    """Each frame's state, renumbered by the states' first frames."""
    _, first = np.unique(state, return_index=True)
    return np.argsort(np.argsort(first))[state]


def results_tuple(r):
    assert r.labels.dtype == r.core_sample_indices.dtype == r.sizes.dtype == r.n_neighbours.dtype == np.int64
    assert r.n_clusters == len(r.sizes) and r.n_frames == len(r.labels) == len(r.frames) == len(r.n_neighbours)
    assert np.array_equal(r.sizes, np.bincount(r.labels[r.labels >= 0], minlength=r.n_clusters))
    assert r.n_noise == int((r.labels < 0).sum()) and r.n_rounds >= 1
    return r.labels, r.core_sample_indices, r.n_clusters


@pytest.mark.parametrize("name", list(TRAJ_CASES))
def test_dbscan_of_a_trajectory(name):
    import torch

    from rmsf_amd import DBSCAN
    x, state, kw = traj_kw(name)
    d = traj_matrix(name)
    ref = dbscan_reference(d, EPS, MIN_SAMPLES)
    dev = torch.tensor(x, device="cuda:0")
    r = DBSCAN(dev, eps=EPS, min_samples=MIN_SAMPLES, **kw).run().results
    assert_same(results_tuple(r), ref)
    assert r.dist_matrix is None and np.array_equal(r.frames, np.arange(N_FRAMES)) and r.matrix_form == "f64"
    # the four planted states, each one cluster, numbered by their first frames; nobody is noise
    assert r.n_clusters == N_STATES and r.n_noise == 0
    assert np.array_equal(r.labels, first_appearance_rank(state))
    assert np.array_equal(r.n_neighbours, (d <= EPS).sum(1))
    # the two routes to the bits give the same results
    for route in ("f64", "bits"):
        rr = DBSCAN(dev, eps=EPS, min_samples=MIN_SAMPLES, matrix=route, **kw).run().results
        assert rr.matrix_form == route
        assert_same(results_tuple(rr), ref)
        assert np.array_equal(rr.n_neighbours, r.n_neighbours) and rr.n_rounds == r.n_rounds
    # a host trajectory, and the matrix on request: DistanceMatrix's own bits
    rk = DBSCAN(x, eps=EPS, min_samples=MIN_SAMPLES, keep_matrix=True, **kw).run().results
    assert_same(results_tuple(rk), ref)
    assert rk.dist_matrix.shape == d.shape and np.array_equal(rk.dist_matrix.view(np.uint64), d.view(np.uint64))


def test_dbscan_of_a_matrix_in_its_four_forms():
    import torch

    from rmsf_amd import DBSCAN, DistanceMatrix
    x, _, kw = traj_kw("gathered")
    d = traj_matrix("gathered")
    dev = torch.tensor(x, device="cuda:0")
    fresh = DistanceMatrix(dev, **kw)                                         # not run yet: run here
    ran = DistanceMatrix(dev, **kw).run()
    for m in (MIN_SAMPLES, 31):                                               # at 31 the smallest state (30) is noise
        ref = dbscan_reference(d, EPS, m)
        for inp in (fresh, ran, np.array(d), torch.tensor(d, device="cuda:0")):
            r = DBSCAN(inp, eps=EPS, min_samples=m).run().results
            assert_same(results_tuple(r), ref)
            assert np.array_equal(r.frames, np.arange(N_FRAMES)) and r.dist_matrix is None
    assert ref[2] == N_STATES - 1 and (ref[0] < 0).sum() == 30
    assert fresh.results.dist_matrix is not None
    lop = torch.tensor(d, device="cuda:0")
    lop[2, 7] = 99.0 if d[2, 7] <= EPS else 0.0                               # neighbours one way only
    with pytest.raises(ValueError, match="not symmetric"):
        DBSCAN(lop, eps=EPS).run()
    for empty, run_kw in ((np.zeros((0, 0)), {}), (torch.zeros((0, 0), dtype=torch.float64, device="cuda:0"), {}),
                          (x, dict(frames=[]))):                              # no frames: empty results
        r = DBSCAN(empty, eps=EPS).run(**run_kw).results
        assert r.n_clusters == 0 and r.n_frames == 0 and r.n_noise == 0
        assert len(r.labels) == len(r.core_sample_indices) == len(r.sizes) == len(r.n_neighbours) == 0


def test_dbscan_of_scattered_frames():
    import torch

    from rmsf_amd import DBSCAN
    x, state, kw = traj_kw("dense")
    d = traj_matrix("dense")
    rows = np.sort(np.random.default_rng(5).permutation(N_FRAMES)[:97])
    assert len(set(np.diff(rows))) > 1                                        # no constant step
    r = DBSCAN(torch.tensor(x, device="cuda:0"), eps=EPS, min_samples=MIN_SAMPLES, **kw).run(
        frames=rows.tolist()).results
    assert np.array_equal(r.frames, rows) and r.n_frames == 97
    # every pair of the sub-matrix is the same pair of the full one: its reference is the full matrix's rows
    assert_same(results_tuple(r), dbscan_reference(d[np.ix_(rows, rows)], EPS, MIN_SAMPLES))
    assert r.n_clusters == N_STATES and np.array_equal(r.labels, first_appearance_rank(state[rows]))


def test_a_frame_with_a_nan_coordinate_is_noise():
    import torch

    from rmsf_amd import DBSCAN
    x, state, kw = traj_kw("dense")
    q = 41
    bad = np.array(x)
    bad[q, 3, 1] = np.nan
    for route in ("f64", "bits"):
        r = DBSCAN(torch.tensor(bad, device="cuda:0"), eps=EPS, min_samples=MIN_SAMPLES, matrix=route, **kw).run().results
        assert r.labels[q] == -1 and r.n_noise == 1 and r.n_neighbours[q] == 1 and q not in r.core_sample_indices
        keep = np.arange(N_FRAMES) != q
        assert r.n_clusters == N_STATES and np.array_equal(r.labels[keep], first_appearance_rank(state[keep]))


def test_script_writes_the_same_labels(tmp_path):
    """rmsf_mi355x.py --dbscan beside --dist-matrix: the labels of the matrix it writes."""
    import subprocess
    import sys

    import torch

    from conftest import ROOT
    from rmsf_amd import DistanceMatrix
    from rmsf_amd.engine import Engine
    from rmsf_amd.synth import generate, motion_table
    n_atoms, n_frames, m = 64, 40, 3
    shard = generate(Engine(), n_atoms, 0, n_frames, seed=0, motion=motion_table(1, n_frames))[:n_frames]
    d = DistanceMatrix(shard).run().results.dist_matrix
    for quantile in (0.1, 0.2, 0.05, 0.3, 0.5):                               # an eps that leaves neither all core nor all noise
        eps = float(np.quantile(d[~np.eye(n_frames, dtype=bool)], quantile))
        ref = dbscan_reference(d, eps, m)
        if ref[2] >= 1 and 0 < len(ref[1]) < n_frames:
            break
    else:
        raise AssertionError("no quantile of the distances separates core frames from the rest")
    del shard
    torch.cuda.empty_cache()
    out, dm = str(tmp_path / "labels.npy"), str(tmp_path / "dm.npy")
    r = subprocess.run([sys.executable, f"{ROOT}/mdanalysis-mpi_amd/rmsf_mi355x.py", "--synthetic", str(n_atoms),
                        str(n_frames), "--align", "average", "--dist-matrix", dm, "--dbscan", out, "--dbscan-eps",
                        repr(eps), "--dbscan-min-samples", str(m)], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    labels = np.load(out)
    assert labels.dtype == np.int64 and np.array_equal(labels, dbscan_reference(np.load(dm), eps, m)[0])
    assert np.array_equal(labels, ref[0])
