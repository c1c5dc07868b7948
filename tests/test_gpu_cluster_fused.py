"""GPU tier of the fused neighbour bits: ``rmsf_pairwise_adjacency`` -- the pair
kernel of csrc/pairwise.hip writing ``d <= cutoff`` as bit rows from its
epilogue, the F x F f64 matrix never stored -- against the stored route
(``rmsf_pairwise_rmsd`` then ``rmsf_adjacency_pack``) on the same inputs,
``rmsf_adjacency_count``, and ``Cluster(matrix="bits" | "auto")`` end to end.

Both routes inline the same distance code and the library is built without
floating-point contraction, so the fused words must be the stored route's word
for word: everything is compared for equality and no tolerance appears."""
import subprocess
import sys

import numpy as np
import pytest

from test_clustering_host import adjacency, assert_same, gromos_reference, pack_reference, points
from test_gpu_clustering import N_FRAMES, N_STATES, RADIUS, TRAJ_CASES, results_tuple, traj_kw, traj_reference
from test_gpu_pairwise import data, selection, weights_of

pytestmark = pytest.mark.gpu

POISON = np.uint64(2 ** 64 - 1)
# (frames, atoms): the smallest inputs; one tile, partial and full; two tiles in one word (two uncovered
# quarters); below and at a full word; a second word with one covered quarter; three words; the end-to-end size
SHAPES = [(1, 3), (2, 3), (15, 4), (16, 17), (17, 33), (63, 20), (64, 20), (65, 20), (130, 33), (130, 20), (300, 50),
          (5, 5000), (70, 3000)]      # 1 tile pair x 157 stages, 15 tile pairs x 94 stages
# Which kernel runs the epilogue is pw_plan's choice (csrc/pairwise.hip): more than one atom range, and with it
# k_pw_fold and a workspace, wherever the atoms fill more than one stage of 32 and the tile pairs do not fill the
# device -- so also at 33 and 50 atoms here; (130, 20) is the three-word shape whose epilogue runs in k_pw_tiles.
FOLDED = {(17, 33), (130, 33), (300, 50), (5, 5000), (70, 3000)}
VARIANTS = {                          # at (130, 33) and (130, 20)
    "gathered": dict(gathered=True),
    "weighted": dict(weighted=True),
    "plain": dict(superpose=False),
    "wide": dict(extra_words=2),
    "cutoff_zero": dict(cutoff=0.0),
    "cutoff_inf": dict(cutoff=float("inf")),
    "zeroing_above": dict(zero_cutoff=1e9),
}


def atom_ranges(n_frames, n_sel):
    """pw_plan's n_ks, restated: stages of 32 atoms over 512 // (tile pairs) ranges at the most."""
    tiles = -(-n_frames // 16)
    stages = max(1, -(-n_sel // 32))
    ks = max(1, min(stages, 512 // (tiles * (tiles + 1) // 2)))
    return -(-stages // -(-stages // ks))


def off_diagonal(d):
    return d[~np.eye(len(d), dtype=bool)]


def median_cutoff(d):
    """The median off-diagonal distance (of the pairs that have one)."""
    off = off_diagonal(d)
    off = off[~np.isnan(off)]
    return float(np.median(off)) if off.size else 0.0


def both_routes(n_frames, n_sel, gathered=False, weighted=False, superpose=True, cutoff=None, zero_cutoff=1e-5,
                extra_words=0, nan_frame=None, fused_calls=1):
    """(matrix, cutoff, stored (words, counts), [fused (words, counts, spare row) per call], workspace bytes):
    centres once, then Engine.pairwise_rmsd + Engine.adjacency_pack, and Engine.pairwise_adjacency into poisoned
    buffers (all-ones words, one row more than needed, counts -5)."""
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    _, sel = selection(n_sel, gathered)
    x = data(n_frames, n_sel, gathered)
    if nan_frame is not None:
        x = x.copy()
        x[nan_frame, (sel[0] if gathered else 0), 1] = np.inf
    x = torch.tensor(x, device="cuda:0")
    sel_dev = eng.sel_tensor(sel)
    w = weights_of(n_sel) if weighted else None
    w_dev = None if w is None else torch.tensor(w, device="cuda:0")
    w_total = float(n_sel) if w is None else float(w.sum())
    centre, g = eng.pairwise_centres(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, w_dev, superpose)
    need = eng.pairwise_workspace_bytes(n_frames, n_sel)
    work = eng.empty(need // 8) if need else None
    args = (x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, w_dev, w_total, centre, g)
    m = torch.full((n_frames, n_frames), float("nan"), dtype=torch.float64, device="cuda:0")
    eng.pairwise_rmsd(*args, m, superpose=superpose, cutoff=zero_cutoff, work=work)
    torch.cuda.synchronize()
    d = m.cpu().numpy()
    cut = median_cutoff(d) if cutoff is None else cutoff
    nw = eng.adjacency_words(n_frames)
    adj, count = eng.adjacency_pack(m, cut, ldw=nw + extra_words)
    stored = adj.cpu().numpy().view(np.uint64), count.cpu().numpy()
    fused = []
    for _ in range(fused_calls):
        adj = torch.full((n_frames + 1, nw + extra_words), -1, dtype=torch.int64, device="cuda:0")
        count = torch.full((n_frames + 1,), -5, dtype=torch.int32, device="cuda:0")
        eng.pairwise_adjacency(*args, adj, count, cut, superpose=superpose, zero_cutoff=zero_cutoff, work=work)
        torch.cuda.synchronize()
        words = adj.cpu().numpy().view(np.uint64)
        counts = count.cpu().numpy()
        assert counts[n_frames] == -5
        fused.append((words[:n_frames], counts[:n_frames], words[n_frames]))
    return d, cut, stored, fused, need


def assert_fused_is_stored(n_frames, d, cut, stored, fused, extra_words=0):
    nw = (n_frames + 63) // 64
    words, counts, spare = fused
    assert words.shape == stored[0].shape == (n_frames, nw + extra_words)
    assert np.all(spare == POISON), "a row >= n was written"
    assert np.all(words[:, nw:] == POISON), "a word past the row's last was written"
    assert np.array_equal(words[:, :nw], stored[0][:, :nw]), "the words of the two routes differ"
    assert counts.dtype == np.int32 and np.array_equal(counts, stored[1]), "the counts of the two routes differ"
    ref_words, ref_counts = pack_reference(d, cut)
    assert np.array_equal(words[:, :nw], ref_words) and np.array_equal(counts, ref_counts)
    if n_frames % 64:                                                        # 2. bits j >= n of the last word are zero
        assert not (words[:, nw - 1] >> np.uint64(n_frames % 64)).any()


# ---- 1., 2. words, counts and tail bits, every shape ---------------------------------------
@pytest.mark.parametrize("n_frames,n_sel", SHAPES)
def test_words_and_counts_equal_the_stored_route(n_frames, n_sel):
    d, cut, stored, fused, need = both_routes(n_frames, n_sel)
    assert (need > 0) == (atom_ranges(n_frames, n_sel) > 1) == ((n_frames, n_sel) in FOLDED)   # which kernel ran it
    assert_fused_is_stored(n_frames, d, cut, stored, fused[0])
    if n_frames >= 15:
        with np.errstate(invalid="ignore"):
            near = off_diagonal(d) <= cut
        assert near.any() and not near.all()                                  # set and clear bits both occur


@pytest.mark.parametrize("n_sel", [33, 20])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants_at_three_words(name, n_sel):
    kw = VARIANTS[name]
    n_frames = 130
    d, cut, stored, fused, need = both_routes(n_frames, n_sel, **kw)
    assert (need > 0) == (n_sel == 33)
    assert_fused_is_stored(n_frames, d, cut, stored, fused[0], extra_words=kw.get("extra_words", 0))
    bits = np.unpackbits(fused[0][0][:, :3].copy().view(np.uint8), axis=1, bitorder="little")[:, :n_frames].astype(bool)
    eye = np.eye(n_frames, dtype=bool)
    if name == "cutoff_zero":
        # the duplicated pair (frame F-1 is frame 0) is under the zeroing cutoff; nothing else is at distance 0
        assert np.array_equal(bits, eye | (d == 0.0)) and bits.sum() == n_frames + 2
    if name == "cutoff_inf":
        assert bits.all() and np.all(fused[0][1] == n_frames)
        assert np.all(fused[0][0][:, 2] == np.uint64((1 << (n_frames - 128)) - 1))
    if name == "zeroing_above":
        assert not d.any() and bits.all()                                     # every distance was stored as 0
    if name in ("gathered", "weighted", "plain", "wide"):
        assert (bits & ~eye).any() and not (bits | eye).all()


# ---- 3. a frame with a non-finite coordinate ----------------------------------------------
def test_nan_frame_is_nobodys_neighbour():
    n_frames, n_sel, q = 130, 33, 70
    d, cut, stored, fused, _ = both_routes(n_frames, n_sel, nan_frame=q)
    assert np.isnan(d[q, np.arange(n_frames) != q]).all() and cut > 0.0
    assert_fused_is_stored(n_frames, d, cut, stored, fused[0])
    words, counts, _ = fused[0]
    row = np.zeros(3, dtype=np.uint64)
    row[q // 64] = np.uint64(1) << np.uint64(q % 64)
    assert np.array_equal(words[q], row) and counts[q] == 1
    assert not ((words[:, q // 64] >> np.uint64(q % 64)) & np.uint64(1))[np.arange(n_frames) != q].any()
    # and no other frame is changed by it
    clean = both_routes(n_frames, n_sel, cutoff=cut)[3][0][0]
    mask = np.full(3, POISON)
    mask[q // 64] ^= np.uint64(1) << np.uint64(q % 64)
    others = np.arange(n_frames) != q
    assert np.array_equal(words[others] & mask, clean[others] & mask)


# ---- 4. a second call ---------------------------------------------------------------------
@pytest.mark.parametrize("n_frames,n_sel", [(130, 20), (70, 3000)])
def test_a_second_call_gives_the_same_bytes(n_frames, n_sel):
    fused = both_routes(n_frames, n_sel, fused_calls=2)[3]
    assert fused[0][0].tobytes() == fused[1][0].tobytes() and fused[0][1].tobytes() == fused[1][1].tobytes()


# ---- more tile pairs than one launch takes ---------------------------------------------------
def test_more_tile_pairs_than_a_launch_takes():
    """93,000 frames are 16.9 M tile pairs; 2^32 / 256 = 16.8 M workgroups is what one launch runs in full (a
    larger grid is not refused: its count wraps).  Five 4-atom structures, each frame one of them moved rigidly:
    frames are neighbours exactly when they show the same structure, so every word is known without a matrix."""
    import torch

    from rmsf_amd.engine import Engine
    from test_gpu_pairwise import reference_sq
    n_frames, n_sel, n_states, cut = 93_000, 4, 5, 0.5
    assert (-(-n_frames // 16)) * (-(-n_frames // 16) + 1) // 2 > 2 ** 32 // 256
    rng = np.random.default_rng(93)
    base = rng.uniform(0.0, 10.0, size=(n_states, n_sel, 3)).astype(np.float32)
    sq, _ = reference_sq(base, None, True)
    assert np.sqrt(np.abs(off_diagonal(sq))).min() > 2 * cut                  # different structures are far apart
    state = rng.integers(0, n_states, size=n_frames)
    x = base[state] + rng.uniform(-5.0, 5.0, size=(n_frames, 1, 3)).astype(np.float32)   # f32 rounding: 1e-6 A
    nw = (n_frames + 63) // 64
    rows = np.zeros((n_states, 64 * nw), dtype=bool)
    rows[:, :n_frames] = state[None, :] == np.arange(n_states)[:, None]
    rows = np.packbits(rows, axis=1, bitorder="little").view("<u8").view(np.int64)       # the row of each structure
    eng = Engine(torch.device("cuda", 0))
    dev = torch.tensor(x, device="cuda:0")
    centre, g = eng.pairwise_centres(dev.data_ptr(), dev.stride(0), n_frames, n_sel, None, None, True)
    assert eng.pairwise_workspace_bytes(n_frames, n_sel) == 0
    adj = torch.full((n_frames + 1, nw + 1), -1, dtype=torch.int64, device="cuda:0")
    count = torch.full((n_frames,), -5, dtype=torch.int32, device="cuda:0")
    eng.pairwise_adjacency(dev.data_ptr(), dev.stride(0), n_frames, n_sel, None, None, float(n_sel), centre, g, adj,
                           count, cut, superpose=True, zero_cutoff=1e-5)
    state_dev = torch.tensor(state, device="cuda:0")
    assert torch.equal(adj[:n_frames, :nw], torch.tensor(rows, device="cuda:0")[state_dev])
    assert bool((adj[n_frames] == -1).all()) and bool((adj[:, nw] == -1).all())
    assert torch.equal(count.to(torch.int64), torch.tensor(np.bincount(state, minlength=n_states),
                                                           device="cuda:0")[state_dev])


# ---- 5. rmsf_adjacency_count ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 1000])
def test_adjacency_count(n):
    import torch

    from rmsf_amd.engine import Engine
    words, counts = pack_reference(points(n), 2.0, ldw=(n + 63) // 64 + 3, poison=int(POISON))
    assert np.all(words[:, -3:] == POISON)
    eng = Engine(torch.device("cuda", 0))
    adj = torch.tensor(words.view(np.int64), device="cuda:0")
    got = eng.adjacency_count(adj, n).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, counts)             # the poison words are not counted
    assert np.array_equal(eng.adjacency_count(adj).cpu().numpy(), counts)


# ---- 6. Cluster(matrix="bits"), end to end ------------------------------------------------------
@pytest.mark.parametrize("name", list(TRAJ_CASES))
def test_cluster_bits_of_a_trajectory(name):
    import torch

    from rmsf_amd import Cluster
    x, state, kw = traj_kw(name)
    d, ref = traj_reference(name)
    neighbours = adjacency(d, RADIUS).sum(1).astype(np.int64)
    for inp in (torch.tensor(x, device="cuda:0"), x):
        r = Cluster(inp, cutoff=RADIUS, matrix="bits", **kw).run().results
        f = Cluster(inp, cutoff=RADIUS, matrix="f64", **kw).run().results
        assert_same(results_tuple(r), ref[:3])
        assert_same(results_tuple(r), results_tuple(f))
        assert r.matrix_form == "bits" and f.matrix_form == "f64"
        assert r.n_neighbours.dtype == f.n_neighbours.dtype == np.int64
        assert np.array_equal(r.n_neighbours, f.n_neighbours) and np.array_equal(r.n_neighbours, neighbours)
        assert r.dist_matrix is None and np.array_equal(r.frames, np.arange(N_FRAMES))
        assert r.n_clusters == N_STATES and r.sizes.tolist() == [120, 90, 60, 30]


def test_cluster_bits_of_scattered_frames_and_of_none():
    import torch

    from rmsf_amd import Cluster
    x, state, kw = traj_kw("dense")
    d, _ = traj_reference("dense")
    rows = np.sort(np.random.default_rng(5).permutation(N_FRAMES)[:97])
    assert len(set(np.diff(rows))) > 1                                        # no constant step
    r = Cluster(torch.tensor(x, device="cuda:0"), cutoff=RADIUS, matrix="bits", **kw).run(frames=rows.tolist()).results
    assert np.array_equal(r.frames, rows) and r.n_frames == 97 and r.matrix_form == "bits"
    sub = d[np.ix_(rows, rows)]
    assert_same(results_tuple(r), gromos_reference(sub, RADIUS)[:3])
    assert np.array_equal(r.n_neighbours, adjacency(sub, RADIUS).sum(1))
    e = Cluster(x, cutoff=RADIUS, matrix="bits").run(frames=[]).results
    assert e.n_clusters == 0 and e.n_frames == 0 and e.dist_matrix is None
    assert len(e.labels) == len(e.centres) == len(e.sizes) == len(e.n_neighbours) == len(e.frames) == 0


# ---- 7. what "auto" takes ---------------------------------------------------------------------
def test_auto_takes_the_bits_only_where_the_matrix_does_not_fit(monkeypatch):
    import torch

    from rmsf_amd import Cluster
    x, _, kw = traj_kw("dense")
    _, ref = traj_reference("dense")
    dev = torch.tensor(x, device="cuda:0")
    matrix_bytes, bit_bytes, dense_bytes = 8 * N_FRAMES ** 2, N_FRAMES * 5 * 8, x.nbytes
    total = torch.cuda.mem_get_info()[1]
    # the true values: nothing that runs today changes its route
    assert Cluster(dev, cutoff=RADIUS, **kw).run().results.matrix_form == "f64"
    # free HBM under twice the matrix, far above twice the bits and the dense copy
    free = matrix_bytes
    assert 2 * (bit_bytes + dense_bytes) < free < 2 * matrix_bytes
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (free, total))
    for inp in (dev, x):
        r = Cluster(inp, cutoff=RADIUS, **kw).run().results
        assert r.matrix_form == "bits"
        assert_same(results_tuple(r), ref[:3])
        with pytest.raises(MemoryError, match=str(matrix_bytes)):
            Cluster(inp, cutoff=RADIUS, matrix="f64", **kw).run()
    # under twice the bits: nothing fits, and the message says what the bits need
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2 * bit_bytes - 2, total))
    for form in ("auto", "bits", "f64"):
        with pytest.raises(MemoryError, match=str(bit_bytes)):
            Cluster(dev, cutoff=RADIUS, matrix=form, **kw).run()


# ---- 8. the script ----------------------------------------------------------------------------
def test_script_writes_the_same_labels_on_both_routes(tmp_path):
    """rmsf_mi355x.py --cluster --cluster-matrix bits beside f64: equal label files."""
    import torch

    from conftest import ROOT
    from rmsf_amd import DistanceMatrix
    from rmsf_amd.engine import Engine
    from rmsf_amd.synth import generate, motion_table
    n_atoms, n_frames = 64, 40
    shard = generate(Engine(), n_atoms, 0, n_frames, seed=0, motion=motion_table(1, n_frames))[:n_frames]
    d = DistanceMatrix(shard).run().results.dist_matrix
    cut = float(np.quantile(off_diagonal(d), 0.25))
    ref = gromos_reference(d, cut)
    assert 1 < len(ref[1]) < n_frames and ref[2][0] >= 2                      # neither one cluster nor all alone
    del shard
    torch.cuda.empty_cache()
    labels = {}
    for form, said in (("bits", "no matrix stored"), ("f64", "stored f64 matrix")):
        out = str(tmp_path / f"labels_{form}.npy")
        r = subprocess.run([sys.executable, f"{ROOT}/mdanalysis-mpi_amd/rmsf_mi355x.py", "--synthetic", str(n_atoms),
                            str(n_frames), "--align", "average", "--cluster", out, "--cluster-cutoff", repr(cut),
                            "--cluster-matrix", form], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        assert said in r.stdout, r.stdout
        labels[form] = np.load(out)
    assert labels["bits"].dtype == np.int64 and np.array_equal(labels["bits"], labels["f64"])
    assert np.array_equal(labels["bits"], ref[0])
