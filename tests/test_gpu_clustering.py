"""GPU tier of the GROMOS clustering (csrc/clustering.hip): the pack of an f64
matrix into neighbour bits, the pick / decrement loop, and ``Cluster`` end to
end, against the numpy restatement of the definition in
tests/test_clustering_host.py and against ``rmsf_cluster_gromos_host``.

Everything after the threshold is integers: labels, centres, sizes and bit
words are compared for equality, and no tolerance appears anywhere.  Where a
trajectory is clustered, the reference runs on ``DistanceMatrix``'s own matrix
of the same input -- the same kernel on the same inputs, reproducible bit for
bit, so no threshold can flip; the matrix kernel is not under test here."""
import functools

import numpy as np
import pytest

from test_clustering_host import (CUT, assert_consequences, assert_nan_frame_alone, assert_same, gromos_reference,
                                  host_cluster, lattice, nan_case, pack_reference, points)

pytestmark = pytest.mark.gpu

POISON = 2 ** 64 - 1
SIZES = [1, 63, 64, 65, 130, 1000]
GENERATORS = {"points": points, "lattice": lattice}


@functools.lru_cache(maxsize=None)
def case(kind: str, n: int):
    """(matrix, cutoff, reference) of a named case; computed once, read-only."""
    if kind in GENERATORS:
        d, cut = GENERATORS[kind](n), CUT
    elif kind == "zero":
        d, cut = points(n), 0.0
    elif kind == "inf":
        d, cut = points(n), float("inf")
    elif kind == "nan":
        d, cut = nan_case(n)[0], CUT
    d.setflags(write=False)
    ref = gromos_reference(d, cut)
    for a in ref:
        a.setflags(write=False)
    return d, cut, ref


def device_pack(d, cut, ld=None, ldw=None):
    """rmsf_adjacency_pack into a poisoned buffer -> (uint64 [n, ldw], int32 [n])."""
    import torch

    from rmsf_amd import _lib
    n = d.shape[0]
    ld = n if ld is None else ld
    m = np.zeros((n, ld))
    m[:, :n] = d
    nw = _lib.load().rmsf_adjacency_words(n)
    ldw = nw if ldw is None else ldw
    dev = torch.tensor(m, device="cuda:0")
    adj = torch.full((n, ldw), -1, dtype=torch.int64, device="cuda:0")       # all-ones words
    count = torch.full((n,), -5, dtype=torch.int32, device="cuda:0")
    _lib.call("rmsf_adjacency_pack", dev.data_ptr(), n, ld, float(cut), adj.data_ptr(), ldw, count.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return adj.cpu().numpy().view(np.uint64), count.cpu().numpy()


def device_cluster(d, cut):
    """Engine.adjacency_pack + Engine.cluster_gromos -> int64 (labels, centres, sizes), and the count tensors."""
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    adj, count = eng.adjacency_pack(torch.tensor(d, device="cuda:0"), cut)
    before = count.clone()
    out = eng.cluster_gromos(adj, count)
    first = tuple(t.cpu().numpy() for t in out)
    again = tuple(t.cpu().numpy() for t in eng.cluster_gromos(adj, count))
    for a, b in zip(first, again):
        assert a.dtype == np.int32 and a.tobytes() == b.tobytes()            # a second run: the same bytes
    assert torch.equal(count, before)                                         # d_count is read, not changed
    return tuple(a.astype(np.int64) for a in first)


# ---- pack ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["points", "lattice"])
def test_pack(kind, n):
    d, cut, _ = case(kind, n)
    words, counts = device_pack(d, cut)
    ref_words, ref_counts = pack_reference(d, cut)
    assert np.array_equal(words, ref_words) and np.array_equal(counts, ref_counts)
    tail = n % 64
    if tail:
        assert not (words[:, -1] >> np.uint64(tail)).any()                    # bits j >= n are zero


def test_pack_wide_rows_keep_their_poison():
    d, cut, _ = case("points", 130)
    words, counts = device_pack(d, cut, ldw=5)                                # 3 words needed
    ref_words, ref_counts = pack_reference(d, cut, ldw=5, poison=POISON)
    assert np.array_equal(words, ref_words) and np.array_equal(counts, ref_counts)
    assert np.all(words[:, 3:] == np.uint64(POISON))


def test_pack_padded_matrix():
    d, cut, _ = case("lattice", 65)
    words, counts = device_pack(d, cut, ld=65 + 3)                            # the 0.0 padding is not read
    ref_words, ref_counts = pack_reference(d, cut)
    assert np.array_equal(words, ref_words) and np.array_equal(counts, ref_counts)


def test_pack_nan_row_sets_only_its_diagonal():
    d, cut, _ = case("nan", 130)
    q = nan_case(130)[2]
    words, counts = device_pack(d, cut)
    ref_words, ref_counts = pack_reference(d, cut)
    assert np.array_equal(words, ref_words) and np.array_equal(counts, ref_counts)
    row = np.zeros(3, dtype=np.uint64)
    row[q // 64] = np.uint64(1) << np.uint64(q % 64)
    assert np.array_equal(words[q], row) and counts[q] == 1
    assert not ((words[:, q // 64] >> np.uint64(q % 64)) & np.uint64(1))[np.arange(130) != q].any()


# ---- the loop -----------------------------------------------------------------------
LOOP_CASES = ([(k, n) for k in ("points", "lattice") for n in SIZES]
              + [("points", 4097), ("zero", 130), ("inf", 130), ("nan", 130)])


@pytest.mark.parametrize("kind,n", LOOP_CASES)
def test_loop(kind, n):
    d, cut, ref = case(kind, n)
    sizes = ref[2]
    if kind == "points" and n >= 63:
        assert (sizes >= 2).sum() >= 3 and (sizes == 1).sum() >= 1
    if kind == "points" and n == 4097:
        assert len(sizes) > 64                                                # several batches of 32
    if kind == "lattice" and n >= 63:
        assert ref[3].any()                                                   # tied picks
    if kind == "zero":
        assert np.array_equal(ref[0], np.arange(n)) and len(sizes) == n
    if kind == "inf":
        assert sizes.tolist() == [n] and ref[1].tolist() == [0]
    got = device_cluster(d, cut)
    assert_same(got, ref[:3])
    assert_same(got, host_cluster(d, cut))
    assert_consequences(*got)
    if kind == "nan":
        _, small, q, keep = nan_case(n)
        assert_nan_frame_alone(got, gromos_reference(small, cut), q, keep)


# ---- Cluster, end to end ------------------------------------------------------------------
N_FRAMES, N_STATES = 300, 4
STATE_SIGMA, NOISE = 2.0, 0.3
RADIUS, MARGIN = 1.5, 0.1


@functools.lru_cache(maxsize=None)
def make_states(n_atoms: int, seed: int = 0):
    """(f32 [F, n_atoms, 3], state of each frame): the generator of
    tests/test_gpu_pairwise.py with four base conformations in place of its
    planted modes -- a base structure plus each state's own displacement of
    2 A per atom, 0.3 A noise, then a random rotation about the centroid and a
    translation per frame; populations 120 / 90 / 60 / 30, shuffled."""
    rng = np.random.default_rng(1000 * seed + 7 * n_atoms + N_FRAMES)
    base = rng.uniform(0.0, 100.0, size=(n_atoms, 3))
    disp = rng.normal(size=(N_STATES, n_atoms, 3))
    disp /= np.sqrt((disp ** 2).sum(axis=(1, 2), keepdims=True) / n_atoms)    # unit displacement per atom
    state = rng.permutation(np.repeat(np.arange(N_STATES), (120, 90, 60, 30)))
    x = base + STATE_SIGMA * disp[state] + NOISE * rng.normal(size=(N_FRAMES, n_atoms, 3))
    q = rng.normal(size=(N_FRAMES, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, a, b, c = q.T
    rot = np.stack([np.stack([1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)], -1),
                    np.stack([2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)], -1),
                    np.stack([2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)], -1)], -2)
    cen = x.mean(axis=1, keepdims=True)
    x = np.einsum("fac,fcd->fad", x - cen, rot) + cen + rng.uniform(-5.0, 5.0, size=(N_FRAMES, 1, 3))
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    state.setflags(write=False)
    return x, state


TRAJ_CASES = {"dense": (50, False, False), "gathered": (33, True, False), "weighted": (50, False, True)}


def traj_kw(name):
    n_sel, gathered, weighted = TRAJ_CASES[name]
    n_atoms, sel = (3 * n_sel, np.arange(1, 3 * n_sel, 3)) if gathered else (n_sel, None)
    w = np.random.default_rng(n_sel).uniform(1.0, 16.0, size=n_sel) if weighted else None
    x, state = make_states(n_atoms)
    return x, state, dict(select=sel, weights=w)


@functools.lru_cache(maxsize=None)
def traj_reference(name):
    """(DistanceMatrix's matrix of the case, its GROMOS reference at RADIUS)."""
    import torch

    from rmsf_amd import DistanceMatrix
    x, state, kw = traj_kw(name)
    d = DistanceMatrix(torch.tensor(x, device="cuda:0"), **kw).run().results.dist_matrix
    same = state[:, None] == state[None, :]
    off = ~np.eye(N_FRAMES, dtype=bool)
    assert d[same & off].max() < RADIUS - MARGIN and d[~same].min() > RADIUS + MARGIN, (
        d[same & off].max(), d[~same].min())
    d.setflags(write=False)
    return d, gromos_reference(d, RADIUS)


def results_tuple(r):
    assert r.labels.dtype == r.centres.dtype == r.sizes.dtype == np.int64
    assert r.n_clusters == len(r.centres) == len(r.sizes) and r.n_frames == len(r.labels) == len(r.frames)
    return r.labels, r.centres, r.sizes


@pytest.mark.parametrize("name", list(TRAJ_CASES))
def test_cluster_of_a_trajectory(name):
    import torch

    from rmsf_amd import Cluster
    x, state, kw = traj_kw(name)
    d, ref = traj_reference(name)
    r = Cluster(torch.tensor(x, device="cuda:0"), cutoff=RADIUS, **kw).run().results
    assert_same(results_tuple(r), ref[:3])
    assert r.dist_matrix is None and np.array_equal(r.frames, np.arange(N_FRAMES))
    # the four planted states, each one cluster, the most populated first
    assert r.n_clusters == N_STATES and r.sizes.tolist() == [120, 90, 60, 30]
    for k in range(N_STATES):
        assert len(set(state[r.labels == k])) == 1
    assert len(set(state[r.centres])) == N_STATES
    # a host trajectory, and the matrix on request: DistanceMatrix's own bits
    rk = Cluster(x, cutoff=RADIUS, keep_matrix=True, **kw).run().results
    assert_same(results_tuple(rk), ref[:3])
    assert rk.dist_matrix.shape == d.shape and np.array_equal(rk.dist_matrix.view(np.uint64), d.view(np.uint64))


def test_cluster_of_a_matrix_in_its_three_forms():
    import torch

    from rmsf_amd import Cluster, DistanceMatrix
    x, _, kw = traj_kw("gathered")
    d, ref = traj_reference("gathered")
    dev = torch.tensor(x, device="cuda:0")
    fresh = DistanceMatrix(dev, **kw)                                         # not run yet: run here
    ran = DistanceMatrix(dev, **kw).run()
    for inp in (fresh, ran, np.array(d), torch.tensor(d, device="cuda:0")):
        r = Cluster(inp, cutoff=RADIUS).run().results
        assert_same(results_tuple(r), ref[:3])
        assert np.array_equal(r.frames, np.arange(N_FRAMES)) and r.dist_matrix is None
    assert fresh.results.dist_matrix is not None
    lop = torch.tensor(d, device="cuda:0")
    lop[2, 7] = 99.0 if d[2, 7] <= RADIUS else 0.0                            # neighbours one way only
    with pytest.raises(ValueError, match="not symmetric"):
        Cluster(lop, cutoff=RADIUS).run()
    for empty, run_kw in ((np.zeros((0, 0)), {}), (torch.zeros((0, 0), dtype=torch.float64, device="cuda:0"), {}),
                          (x, dict(frames=[]))):                              # no frames: empty results
        r = Cluster(empty, cutoff=RADIUS).run(**run_kw).results
        assert r.n_clusters == 0 and r.n_frames == 0 and len(r.labels) == len(r.centres) == len(r.sizes) == 0


def test_cluster_of_scattered_frames():
    import torch

    from rmsf_amd import Cluster
    x, state, kw = traj_kw("dense")
    d, _ = traj_reference("dense")
    rows = np.sort(np.random.default_rng(5).permutation(N_FRAMES)[:97])
    assert len(set(np.diff(rows))) > 1                                        # no constant step
    r = Cluster(torch.tensor(x, device="cuda:0"), cutoff=RADIUS, **kw).run(frames=rows.tolist()).results
    assert np.array_equal(r.frames, rows) and r.n_frames == 97
    # every pair of the sub-matrix is the same pair of the full one: its reference is the full matrix's rows
    ref = gromos_reference(d[np.ix_(rows, rows)], RADIUS)
    assert_same(results_tuple(r), ref[:3])
    assert r.n_clusters == N_STATES
    for k in range(N_STATES):
        assert len(set(state[r.frames[r.labels == k]])) == 1


def test_script_writes_the_same_labels(tmp_path):
    """rmsf_mi355x.py --cluster beside --dist-matrix: the labels of the matrix it writes."""
    import subprocess
    import sys

    import torch

    from conftest import ROOT
    from rmsf_amd import DistanceMatrix
    from rmsf_amd.engine import Engine
    from rmsf_amd.synth import generate, motion_table
    n_atoms, n_frames = 64, 40
    shard = generate(Engine(), n_atoms, 0, n_frames, seed=0, motion=motion_table(1, n_frames))[:n_frames]
    d = DistanceMatrix(shard).run().results.dist_matrix
    cut = float(np.quantile(d[~np.eye(n_frames, dtype=bool)], 0.25))
    ref = gromos_reference(d, cut)
    assert 1 < len(ref[1]) < n_frames and ref[2][0] >= 2                      # neither one cluster nor all alone
    del shard
    torch.cuda.empty_cache()
    out, dm = str(tmp_path / "labels.npy"), str(tmp_path / "dm.npy")
    r = subprocess.run([sys.executable, f"{ROOT}/mdanalysis-mpi_amd/rmsf_mi355x.py", "--synthetic", str(n_atoms),
                        str(n_frames), "--align", "average", "--dist-matrix", dm, "--cluster", out,
                        "--cluster-cutoff", repr(cut)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    labels = np.load(out)
    assert labels.dtype == np.int64 and np.array_equal(labels, gromos_reference(np.load(dm), cut)[0])
    assert np.array_equal(labels, ref[0])
