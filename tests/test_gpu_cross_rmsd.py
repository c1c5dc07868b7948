"""GPU tier: the cross RMSD matrix d[i, j] = RMSD(A_i, B_j) (csrc/pairwise.hip,
the rectangle's ``k_pw_tiles`` / ``k_pw_fold``), ``rmsf_row_argmin`` and
``CrossDistanceMatrix``, against a numpy f64 reference that does not use QCP:

  * superposition on: weighted centring of either side, ``H = (w d_Bj)^T
    d_Ai``, an SVD with the determinant sign, ``d^2 = (G_i + G_j - 2 (s0 + s1
    +- s2)) / sum w``;
  * superposition off: the direct ``sum w |x_Ai - x_Bj|^2 / sum w``.

Data: the generator of tests/test_gpu_pairwise.py (restated here): one
trajectory of F_a + F_b frames, A its first F_a frames, B the rest, B's last
frame overwritten by A's frame 0 -- one planted duplicate pair (0, F_b - 1).

Bound (derived, not measured; the derivation is in tests/test_gpu_pairwise.py's
docstring and DESIGN section 4 -- the arithmetic is the square kernel's):
``|d^2_gpu - d^2_ref| <= 1e-12 S_ij``, ``S_ij = (G_i + G_j) / (2 sum w)`` with
G about each frame's own weighted centre.  Every pair is compared except the
planted duplicate, which the default cutoff sets to exactly 0; every compared
reference distance is asserted > 0.1 A.

Worst ratios |d^2 - d^2_ref| / (1e-12 S) measured on an MI355X over the 8
variants of each shape (dense / gathered, unweighted / weighted, superposed /
plain): see DESIGN section 4, "Cross RMSD matrix".
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODE_SIGMA = (2.0, 1.4, 1.0)   # A per atom, the three planted modes
NOISE = 0.3
STAGE = 32                     # atoms the kernel stages at a time (kKA of csrc/pairwise.hip)
BOUND = 1e-12


@functools.lru_cache(maxsize=None)
def make_traj(n_atoms: int, n_frames: int, seed: int = 0) -> np.ndarray:
    """f32 [F, n_atoms, 3]: base + sum_k a_k(f) mode_k + noise, then a random
    rotation about the centroid and a translation per frame."""
    rng = np.random.default_rng(1000 * seed + 7 * n_atoms + n_frames)
    base = rng.uniform(0.0, 100.0, size=(n_atoms, 3))
    modes = rng.normal(size=(3, n_atoms, 3))
    modes /= np.sqrt((modes ** 2).sum(axis=(1, 2), keepdims=True) / n_atoms)   # unit displacement per atom
    amp = rng.normal(size=(n_frames, 3)) * np.asarray(MODE_SIGMA)
    x = base + np.einsum("fk,kac->fac", amp, modes) + NOISE * rng.normal(size=(n_frames, n_atoms, 3))
    q = rng.normal(size=(n_frames, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, a, b, c = q.T
    rot = np.stack([np.stack([1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)], -1),
                    np.stack([2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)], -1),
                    np.stack([2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)], -1)], -2)
    cen = x.mean(axis=1, keepdims=True)
    x = np.einsum("fac,fcd->fad", x - cen, rot) + cen + rng.uniform(-5.0, 5.0, size=(n_frames, 1, 3))
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def selection(n_sel: int, gathered: bool):
    """(n_atoms of the frame, sel): dense, or every 3rd of 3 n_sel atoms."""
    return (3 * n_sel, np.arange(1, 3 * n_sel, 3)) if gathered else (n_sel, None)


@functools.lru_cache(maxsize=None)
def data(f_a: int, f_b: int, n_sel: int, gathered: bool):
    """(A [F_a, n_atoms, 3], B [F_b, n_atoms, 3]) of a case: the two parts of
    one generated trajectory, B's last frame := A's frame 0."""
    n_atoms, _ = selection(n_sel, gathered)
    x = make_traj(n_atoms, f_a + f_b)
    a, b = x[:f_a].copy(), x[f_a:].copy()
    b[f_b - 1] = a[0]
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def weights_of(n_sel: int):
    w = np.random.default_rng(n_sel).uniform(1.0, 16.0, size=n_sel)
    w.setflags(write=False)
    return w


def reference_sq(xa: np.ndarray, xb: np.ndarray, w, superpose: bool):
    """(d^2 [F_a, F_b], S [F_a, F_b]) of the selected rows xa f32 [F_a, n, 3]
    and xb f32 [F_b, n, 3] in numpy f64; no QCP."""
    xa, xb = xa.astype(np.float64), xb.astype(np.float64)
    n = xa.shape[1]
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    wt = w.sum()
    wc = w[None, :, None]
    da = xa - (wc * xa).sum(axis=1, keepdims=True) / wt
    db = xb - (wc * xb).sum(axis=1, keepdims=True) / wt
    ga, gb = (wc * da * da).sum(axis=(1, 2)), (wc * db * db).sum(axis=(1, 2))
    s_scale = (ga[:, None] + gb[None, :]) / (2.0 * wt)
    if not superpose:
        sq = np.empty((len(xa), len(xb)))
        for i in range(len(xa)):
            diff = xb - xa[i]
            sq[i] = (wc * diff * diff).sum(axis=(1, 2)) / wt
        return sq, s_scale
    h = np.einsum("jac,iad->ijcd", wc * db, da)      # H[i, j] = (w d_Bj)^T d_Ai
    u, s, vt = np.linalg.svd(h)
    sign = np.sign(np.linalg.det(u @ vt))
    tr = s[..., 0] + s[..., 1] + sign * s[..., 2]
    return (ga[:, None] + gb[None, :] - 2.0 * tr) / wt, s_scale


def rows(x: np.ndarray, sel):
    return x if sel is None else x[:, sel]


@functools.lru_cache(maxsize=None)
def reference(f_a: int, f_b: int, n_sel: int, gathered: bool, weighted: bool, superpose: bool):
    _, sel = selection(n_sel, gathered)
    a, b = data(f_a, f_b, n_sel, gathered)
    sq, s = reference_sq(rows(a, sel), rows(b, sel), weights_of(n_sel) if weighted else None, superpose)
    sq.setflags(write=False)
    s.setflags(write=False)
    return sq, s


def check(m: np.ndarray, sq_ref: np.ndarray, s_scale: np.ndarray, dup, label: str) -> float:
    """The duplicate pair exactly 0, every other pair inside the bound;
    returns the largest ratio."""
    assert m.shape == sq_ref.shape and m.dtype == np.float64
    assert not np.isnan(m).any(), "an element was never written"
    skip = np.zeros(m.shape, dtype=bool)
    if dup is not None:
        assert m[dup] == 0.0, f"the duplicate pair is not exactly zero: {m[dup]!r}"
        skip[dup] = True
    keep = ~skip
    assert keep.sum() == m.size - (1 if dup is not None else 0)   # exactly one pair is left out
    # the test's own data: everything compared is a real distance, far above the cutoff
    d_ref = np.sqrt(np.abs(sq_ref))
    assert np.all(d_ref[keep] > 0.1), f"{label}: a non-duplicate reference distance <= 0.1 A"
    ratio = np.abs(m * m - sq_ref) / (BOUND * s_scale)
    worst = float(ratio[keep].max()) if keep.any() else 0.0
    print(f"{label}: max |d2 - d2_ref| / (1e-12 S) = {worst:.3e}")
    assert worst <= 1.0, f"{label}: ratio {worst}"
    return worst


def engine_cross(xa, sel_a, xb, sel_b, w, superpose, cutoff=1e-5, pad=0, sentinel=float("nan")):
    """rmsf_cross_rmsd on host arrays xa [F_a, atoms_a, 3], xb [F_b, atoms_b,
    3] copied to HBM; the whole [F_a, F_b + pad] output buffer comes back."""
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    ta, tb = torch.tensor(xa, device="cuda:0"), torch.tensor(xb, device="cuda:0")
    n_a, n_b = len(xa), len(xb)
    n_sel = xa.shape[1] if sel_a is None else len(sel_a)
    assert n_sel == (xb.shape[1] if sel_b is None else len(sel_b))
    sa, sb = eng.sel_tensor(sel_a), eng.sel_tensor(sel_b)
    w_dev = None if w is None else torch.tensor(w, device="cuda:0")
    w_total = float(n_sel) if w is None else float(w.sum())
    if superpose:
        ca, ga = eng.pairwise_centres(ta.data_ptr(), ta.stride(0), n_a, n_sel, sa, w_dev, True)
        cb, gb = eng.pairwise_centres(tb.data_ptr(), tb.stride(0), n_b, n_sel, sb, w_dev, True)
    else:
        ca, ga = eng.pairwise_centres(ta.data_ptr(), ta.stride(0), n_a, n_sel, sa, w_dev, False)
        cb, gb = eng.pairwise_centres_about(tb.data_ptr(), tb.stride(0), n_b, n_sel, sb, w_dev, ca)
    need = eng.cross_workspace_bytes(n_a, n_b, n_sel)
    work = eng.empty(need // 8) if need else None
    out = torch.full((n_a, n_b + pad), sentinel, dtype=torch.float64, device="cuda:0")
    eng.cross_rmsd(ta.data_ptr(), ta.stride(0), n_a, sa, ca, ga, tb.data_ptr(), tb.stride(0), n_b, sb, cb, gb,
                   n_sel, w_dev, w_total, out, superpose=superpose, cutoff=cutoff, work=work)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def engine_matrix(f_a, f_b, n_sel, gathered, weighted, superpose, cutoff=1e-5):
    _, sel = selection(n_sel, gathered)
    a, b = data(f_a, f_b, n_sel, gathered)
    return engine_cross(a, sel, b, sel, weights_of(n_sel) if weighted else None, superpose, cutoff)


def public(f_a, f_b, n_sel, gathered, weighted, superpose, host=False, run_kw=None, **kw):
    import torch

    from rmsf_amd import CrossDistanceMatrix
    _, sel = selection(n_sel, gathered)
    a, b = data(f_a, f_b, n_sel, gathered)
    if not host:
        a, b = torch.tensor(a, device="cuda:0"), torch.tensor(b, device="cuda:0")
    cm = CrossDistanceMatrix(a, b, select=sel, weights=weights_of(n_sel) if weighted else None,
                             superposition=superpose, **kw).run(**(run_kw or {}))
    return cm.results


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. every shape, engine level and through CrossDistanceMatrix ------------------------
SHAPES = [(1, 1, 3),                                                   # only the duplicate: [[0]]
          (15, 17, 4), (16, 16, 17), (17, 33, 33), (33, 5, 31),       # tile edges, 2 x 3 tiles, rows > columns
          (1, 50, 214), (50, 1, 214),                                  # one frame against many, both ways
          (9, 20, STAGE - 1), (9, 20, STAGE), (9, 20, STAGE + 1),      # atom-stage edges
          (3, 5, 5000)]                                                # one tile pair, 157 atom ranges


def run_case(f_a, f_b, n_sel, gathered, weighted, superpose):
    sq_ref, s = reference(f_a, f_b, n_sel, gathered, weighted, superpose)
    label = f"({f_a} x {f_b} x {n_sel}) gathered={gathered} weighted={weighted} superpose={superpose}"
    m = engine_matrix(f_a, f_b, n_sel, gathered, weighted, superpose)
    worst = check(m, sq_ref, s, (0, f_b - 1), "engine " + label)
    r = public(f_a, f_b, n_sel, gathered, weighted, superpose)
    assert r.n_frames == f_a and r.n_frames_b == f_b
    np.testing.assert_array_equal(r.frames, np.arange(f_a))
    np.testing.assert_array_equal(r.frames_b, np.arange(f_b))
    assert same_bits(r.dist_matrix, m), "CrossDistanceMatrix and the engine differ in their bits"
    return worst


@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("f_a,f_b,n_sel", SHAPES)
def test_matrix_against_reference(f_a, f_b, n_sel, gathered, weighted, superpose):
    run_case(f_a, f_b, n_sel, gathered, weighted, superpose)
    if (f_a, f_b) == (1, 1):
        m = engine_matrix(f_a, f_b, n_sel, gathered, weighted, superpose)
        assert m.shape == (1, 1) and m[0, 0] == 0.0


@pytest.mark.parametrize("weighted,superpose", [(False, True), (True, False)],
                         ids=["unweighted-superpose", "weighted-plain"])
def test_direct_plan_with_many_tile_pairs(weighted, superpose):
    """528 x 130 x 40: 33 x 9 = 297 tile pairs, over the 256 that leave room to
    split: the epilogue runs in the contraction kernel, after 2 stages."""
    import torch

    from rmsf_amd.engine import Engine
    assert Engine(torch.device("cuda", 0)).cross_workspace_bytes(528, 130, 40) == 0
    run_case(528, 130, 40, False, weighted, superpose)


# ---- 2. mixed operands at 17 x 33 x 33 -------------------------------------------------
MIX = (17, 33, 33)


@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("which", ["a_gathered", "b_gathered"])
def test_one_side_gathered_the_other_dense(which, weighted, superpose):
    """One side gathered from frames of 3 n_sel atoms (frame stride 9 n_sel
    floats), the other the same rows as a dense array: the same numbers reach
    the kernel as with both sides gathered, so the same bits come out."""
    f_a, f_b, n_sel = MIX
    _, sel = selection(n_sel, True)
    a, b = data(f_a, f_b, n_sel, True)
    assert a.strides[0] == 4 * 9 * n_sel
    w = weights_of(n_sel) if weighted else None
    sq_ref, s = reference(f_a, f_b, n_sel, True, weighted, superpose)
    if which == "a_gathered":
        m = engine_cross(a, sel, np.ascontiguousarray(b[:, sel]), None, w, superpose)
    else:
        m = engine_cross(np.ascontiguousarray(a[:, sel]), None, b, sel, w, superpose)
    check(m, sq_ref, s, (0, f_b - 1), f"{which} weighted={weighted} superpose={superpose}")
    assert same_bits(m, engine_matrix(f_a, f_b, n_sel, True, weighted, superpose))


@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
def test_different_selections_into_differently_sized_frames(superpose):
    """A's atoms are every 3rd of 99; B's the same coordinates at every 2nd
    row from row 4 of frames of 71 atoms, random numbers between them."""
    f_a, f_b, n_sel = MIX
    _, sel_a = selection(n_sel, True)
    a, b = data(f_a, f_b, n_sel, True)
    sel_b = (np.arange(n_sel) * 2 + 4).astype(np.int64)     # 4, 6, ..., 68 of 71 atoms
    wide = np.random.default_rng(5).uniform(-50.0, 150.0, size=(f_b, 71, 3)).astype(np.float32)
    wide[:, sel_b] = b[:, sel_a]
    sq_ref, s = reference(f_a, f_b, n_sel, True, True, superpose)
    m = engine_cross(a, sel_a, wide, sel_b, weights_of(n_sel), superpose)
    check(m, sq_ref, s, (0, f_b - 1), f"two selections superpose={superpose}")
    assert same_bits(m, engine_matrix(f_a, f_b, n_sel, True, True, superpose))
    # and through CrossDistanceMatrix(select=, select_b=), A in HBM, B on the host
    import torch

    from rmsf_amd import CrossDistanceMatrix
    r = CrossDistanceMatrix(torch.tensor(a, device="cuda:0"), wide, select=sel_a, select_b=sel_b,
                            weights=weights_of(n_sel), superposition=superpose).run().results
    assert same_bits(r.dist_matrix, m)


@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
def test_strided_hbm_tensor_against_a_host_array(superpose):
    """A: every 2nd frame of an HBM tensor, read in place (frame stride 2 x 9
    n_sel floats, gathered); B: a host array, copied dense."""
    import torch

    from rmsf_amd import CrossDistanceMatrix
    f_a, f_b, n_sel = MIX
    _, sel = selection(n_sel, True)
    a, b = data(f_a, f_b, n_sel, True)
    twice = np.random.default_rng(6).uniform(0.0, 100.0, size=(2 * f_a, 3 * n_sel, 3)).astype(np.float32)
    twice[::2] = a
    sq_ref, s = reference(f_a, f_b, n_sel, True, False, superpose)
    r = CrossDistanceMatrix(torch.tensor(twice, device="cuda:0"), b, select=sel,
                            superposition=superpose).run(step=2).results
    np.testing.assert_array_equal(r.frames, np.arange(0, 2 * f_a, 2))
    np.testing.assert_array_equal(r.frames_b, np.arange(f_b))
    check(r.dist_matrix, sq_ref, s, (0, f_b - 1), f"step=2 in place superpose={superpose}")
    assert same_bits(r.dist_matrix, engine_matrix(f_a, f_b, n_sel, True, False, superpose))


# ---- 3. the output buffer -------------------------------------------------------------
@pytest.mark.parametrize("f_a,f_b,n_sel", [(17, 33, 33), (3, 5, 5000), (33, 5, 31)])
def test_padded_output_keeps_its_padding(f_a, f_b, n_sel):
    """ld = F_b + 3: the padding columns keep the sentinel written before the
    call (split-K fold and direct epilogue alike)."""
    a, b = data(f_a, f_b, n_sel, False)
    m = engine_cross(a, None, b, None, None, True, pad=3, sentinel=-7.0)
    assert m.shape == (f_a, f_b + 3)
    assert np.all(m[:, f_b:] == -7.0), "a padding column was written"
    assert same_bits(np.ascontiguousarray(m[:, :f_b]), engine_matrix(f_a, f_b, n_sel, False, False, True))


# ---- 4. the rectangle against itself turned, and against the square matrix -----------------
@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_transpose(weighted, superpose):
    """cross(B, A) = cross(A, B).T to 2e-12 S in d^2: each is within 1e-12 S of
    one reference."""
    f_a, f_b, n_sel = MIX
    a, b = data(f_a, f_b, n_sel, False)
    w = weights_of(n_sel) if weighted else None
    _, s = reference(f_a, f_b, n_sel, False, weighted, superpose)
    ab = engine_cross(a, None, b, None, w, superpose)
    ba = engine_cross(b, None, a, None, w, superpose)
    assert ba.shape == (f_b, f_a)
    ratio = np.abs(ab * ab - (ba * ba).T) / (BOUND * s)
    print(f"transpose weighted={weighted} superpose={superpose}: max ratio {ratio.max():.3e}")
    assert ratio.max() <= 2.0


@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_block_of_the_square_matrix(weighted, superpose):
    """cross(A, B) = DistanceMatrix(A ++ B)[:F_a, F_a:] to 2e-12 S in d^2."""
    import torch

    from rmsf_amd import DistanceMatrix
    f_a, f_b, n_sel = MIX
    a, b = data(f_a, f_b, n_sel, False)
    w = weights_of(n_sel) if weighted else None
    _, s = reference(f_a, f_b, n_sel, False, weighted, superpose)
    cat = torch.tensor(np.concatenate([a, b]), device="cuda:0")
    sq = DistanceMatrix(cat, weights=w, superposition=superpose).run().results.dist_matrix[:f_a, f_a:]
    m = engine_cross(a, None, b, None, w, superpose)
    ratio = np.abs(m * m - sq * sq) / (BOUND * s)
    print(f"square block weighted={weighted} superpose={superpose}: max ratio {ratio.max():.3e}")
    assert ratio.max() <= 2.0


# ---- 5. bits -------------------------------------------------------------------------
@pytest.mark.parametrize("f_a,f_b,n_sel", [(17, 33, 33), (3, 5, 5000), (33, 5, 31)])
def test_two_runs_are_identical_in_bits(f_a, f_b, n_sel):
    x = engine_matrix(f_a, f_b, n_sel, False, True, True)
    y = engine_matrix(f_a, f_b, n_sel, False, True, True)
    assert x is not y and same_bits(x, y)


@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
def test_host_and_hbm_inputs_give_the_same_bits(gathered):
    f_a, f_b, n_sel = MIX
    dev = public(f_a, f_b, n_sel, gathered, True, True)
    host = public(f_a, f_b, n_sel, gathered, True, True, host=True)
    batched = public(f_a, f_b, n_sel, gathered, True, True, host=True, batch_frames=7)
    assert same_bits(dev.dist_matrix, host.dist_matrix) and same_bits(dev.dist_matrix, batched.dist_matrix)
    np.testing.assert_array_equal(dev.nearest, host.nearest)
    assert same_bits(dev.nearest_dist, host.nearest_dist)


@pytest.mark.parametrize("host", [False, True], ids=["hbm", "host"])
def test_frame_lists_against_sliced_inputs(host):
    """run(frames=, frames_b=) gives the bits of the pre-sliced inputs."""
    import torch

    from rmsf_amd import CrossDistanceMatrix
    f_a, f_b, n_sel = 33, 40, 31
    _, sel = selection(n_sel, True)
    a, b = data(f_a, f_b, n_sel, True)
    fa, fb = np.r_[0:10, 20:30, 32], np.r_[3, 5:17, 39]
    to = (lambda x: np.ascontiguousarray(x)) if host else (lambda x: torch.tensor(x, device="cuda:0"))
    r = CrossDistanceMatrix(to(a), to(b), select=sel).run(frames=fa, frames_b=fb).results
    q = CrossDistanceMatrix(to(a[fa]), to(b[fb]), select=sel).run().results
    np.testing.assert_array_equal(r.frames, fa)
    np.testing.assert_array_equal(r.frames_b, fb)
    assert (r.n_frames, r.n_frames_b) == (len(fa), len(fb)) and r.dist_matrix.shape == (len(fa), len(fb))
    assert same_bits(r.dist_matrix, q.dist_matrix)
    np.testing.assert_array_equal(r.nearest, q.nearest)
    assert r.dist_matrix[0, len(fb) - 1] == 0.0     # A's frame 0 and B's last frame: the duplicate is in both lists
    sq_ref, s = reference_sq(a[fa][:, sel], b[fb][:, sel], None, True)
    check(r.dist_matrix, sq_ref, s, (0, len(fb) - 1), f"frames= frames_b= host={host}")
    # start / stop / step go to A alone
    r = CrossDistanceMatrix(to(a), to(b), select=sel).run(4, 30, 5).results
    np.testing.assert_array_equal(r.frames, np.arange(4, 30, 5))
    assert r.dist_matrix.shape == (len(r.frames), f_b)
    assert same_bits(r.dist_matrix, CrossDistanceMatrix(to(a[4:30:5]), to(b), select=sel).run().results.dist_matrix)


def test_one_frame_as_a_2d_array_and_empty_sides():
    import torch

    from rmsf_amd import CrossDistanceMatrix
    f_a, f_b, n_sel = 50, 1, 214
    a, b = data(f_a, f_b, n_sel, False)
    whole = CrossDistanceMatrix(torch.tensor(a, device="cuda:0"), b).run().results
    flat = CrossDistanceMatrix(torch.tensor(a, device="cuda:0"), b[0]).run().results        # [n_atoms, 3]
    assert flat.dist_matrix.shape == (f_a, 1) and same_bits(whole.dist_matrix, flat.dist_matrix)
    turned = CrossDistanceMatrix(torch.tensor(b[0], device="cuda:0"), a).run().results
    assert turned.dist_matrix.shape == (1, f_a) and turned.dist_matrix[0, 0] == 0.0
    for kw, shape in ((dict(frames=[]), (0, f_a)), (dict(frames_b=[]), (1, 0))):
        r = CrossDistanceMatrix(b, a).run(**kw).results
        assert r.dist_matrix.shape == shape and r.dist_matrix.dtype == np.float64
        assert (r.n_frames, r.n_frames_b) == shape and r.nearest.shape == (shape[0],)
        assert r.nearest.dtype == np.int64 and r.nearest_dist.shape == (shape[0],)


# ---- 6. the cutoff ---------------------------------------------------------------------
@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
@pytest.mark.parametrize("f_a,f_b,n_sel", [(17, 33, 33), (3, 5, 5000)])
def test_cutoff_zero_leaves_the_duplicate_raw(f_a, f_b, n_sel, superpose):
    raw = engine_matrix(f_a, f_b, n_sel, False, False, superpose, cutoff=0.0)
    cut = engine_matrix(f_a, f_b, n_sel, False, False, superpose)
    dup = (0, f_b - 1)
    print(f"({f_a} x {f_b} x {n_sel}) superpose={superpose}: raw duplicate distance {raw[dup]:.3e} A")
    assert 0.0 <= raw[dup] < 1e-5 and cut[dup] == 0.0
    raw[dup] = 0.0
    assert same_bits(raw, cut), "the cutoff moved another element"
    r = public(f_a, f_b, n_sel, False, False, superpose, cutoff=0.0)
    assert 0.0 <= r.dist_matrix[dup] < 1e-5


# ---- 7. the row minimum ---------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 5], ids=["tight", "padded"])
@pytest.mark.parametrize("n_cols", [1, 255, 256, 257, 1000])
def test_row_argmin(n_cols, pad):
    """Ties planted at known columns -- within one thread's columns (c and c +
    256), across threads, across the halves of the tree; the padding holds
    smaller values than any entry.  numpy.argmin's answer exactly, the values
    in their bits.  Rows with NaN: numpy.argmin takes a NaN for the least, so
    the first NaN's column and that NaN come back -- at column 0, at the last
    column, at 255, 256 and 300, at two columns of different threads (either
    order of thread and column), in one thread's columns, and beside exact
    zeros on either side."""
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    rng = np.random.default_rng(n_cols)
    ties = [t for t in ([0], [n_cols - 1], [3, 200], [200, 3 + 256], [3, 3 + 256, 3 + 512], [254, 255, 256],
                        [127, 128], [700, 999], [1, 130, 258, 900], list(range(n_cols)))
            if max(t) < n_cols]
    m = rng.uniform(1.0, 2.0, size=(len(ties) + 2, n_cols))
    for row, cols in enumerate(ties):
        m[row, cols] = 0.0 if row % 2 else 0.5          # exact zeros, as the cutoff writes them, and plain ties
    m[len(ties)] = np.inf                               # nothing below +inf: column 0
    nans = [t for t in ([0], [n_cols - 1], [255], [256], [300], [3, 200], [200, 3 + 256], [5, 5 + 256], [254, 255, 256],
                        [127, 128], [999, 1], list(range(n_cols)))
            if max(t) < n_cols]
    zeros = [[], [0], [n_cols - 1], [2, 129, 257]]      # exact zeros beside the NaN: before it, after it, none
    nan_rows = rng.uniform(1.0, 2.0, size=(len(nans) * len(zeros), n_cols))
    first_nan = []
    for k, cols in enumerate(nans):
        for z, zc in enumerate(zeros):
            row = nan_rows[k * len(zeros) + z]
            row[[c for c in zc if c < n_cols]] = 0.0
            row[cols] = np.nan
            first_nan.append(min(cols))
    m = np.concatenate([m, nan_rows, np.full((1, n_cols), np.inf)])
    m[-1, n_cols // 2] = np.nan                         # a NaN among +inf
    first_nan.append(n_cols // 2)
    buf = torch.full((len(m), n_cols + pad), -1.0, dtype=torch.float64, device="cuda:0")
    buf[:, :n_cols] = torch.tensor(m, device="cuda:0")
    idx, val = eng.row_argmin(buf[:, :n_cols])
    torch.cuda.synchronize()
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert idx.dtype == np.int64 and val.dtype == np.float64
    want = np.argmin(m, axis=1)
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(idx[:len(ties)], [t[0] for t in ties])
    np.testing.assert_array_equal(idx[-len(first_nan):], first_nan)
    assert np.isnan(val[-len(first_nan):]).all() and not np.isnan(val[:-len(first_nan)]).any()
    assert same_bits(val, m[np.arange(len(m)), want])


def test_nearest_is_the_argmin_of_the_matrix():
    f_a, f_b, n_sel = 33, 5, 31
    for gathered in (False, True):
        r = public(f_a, f_b, n_sel, gathered, False, True)
        assert r.nearest.dtype == np.int64 and r.nearest.shape == (f_a,)
        np.testing.assert_array_equal(r.nearest, np.argmin(r.dist_matrix, axis=1))
        assert same_bits(r.nearest_dist, r.dist_matrix.min(axis=1))
        assert r.nearest[0] == f_b - 1 and r.nearest_dist[0] == 0.0      # frame 0's duplicate
    # duplicated references: the first of the equal columns
    import torch

    from rmsf_amd import CrossDistanceMatrix
    a, b = data(f_a, f_b, n_sel, False)
    r = CrossDistanceMatrix(torch.tensor(a, device="cuda:0"), np.concatenate([b, b])).run().results
    np.testing.assert_array_equal(r.nearest, np.argmin(r.dist_matrix, axis=1))
    assert r.nearest.max() < f_b and same_bits(r.dist_matrix[:, :f_b], r.dist_matrix[:, f_b:])


# ---- 8. script mode ---------------------------------------------------------------------------
def test_script_cross_rmsd_of_two_xtc_files(tmp_path):
    """rmsf_mi355x.py --cross-rmsd OUT --cross-with B.xtc (GRO topology, no
    MDAnalysis): the matrix CrossDistanceMatrix gives for the two files, the
    selection and the guessed masses."""
    import subprocess
    import sys

    from conftest import ROOT
    from rmsf_amd import CrossDistanceMatrix
    from rmsf_amd.topology import GroTopology, write_gro
    from rmsf_amd.xtc import write_xtc
    n_res, f_a, f_b = 20, 12, 5
    resids = np.repeat(np.arange(1, n_res + 1), 3)
    resnames = np.array(["ALA"] * (3 * n_res))
    names = np.tile(["N", "CA", "C"], n_res)
    x = make_traj(3 * n_res, f_a + f_b)
    gro, xa, xb, out = (str(tmp_path / n) for n in ("s.gro", "a.xtc", "b.xtc", "cross.npy"))
    write_gro(gro, resids, resnames, names, x[0])
    write_xtc(xa, x[:f_a])
    write_xtc(xb, x[f_a:])
    r = subprocess.run([sys.executable, f"{ROOT}/mdanalysis-mpi_amd/rmsf_mi355x.py", "--topology", gro,
                        "--trajectory", xa, "--cross-rmsd", out, "--cross-with", xb], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"cross RMSD matrix, {f_a} x {f_b} frames" in r.stdout
    top = GroTopology(gro)
    sel = top.select("protein and name CA")
    assert len(sel) == n_res
    want = CrossDistanceMatrix(xa, xb, select=sel, weights=top.masses[sel]).run().results.dist_matrix
    got = np.load(out)
    assert got.shape == (f_a, f_b) and same_bits(got, want)
    assert got.min() > 0.1


# ---- the matrix must fit ----------------------------------------------------------------------
def test_matrix_over_half_the_free_hbm_is_refused():
    """200,000 x 200,000 frames: a 320 GB f64 matrix -- a MemoryError stating
    the bytes, before any launch (two 7.2 MB tensors of zero frames are all
    that is allocated)."""
    import torch

    from rmsf_amd import CrossDistanceMatrix
    x = torch.zeros((200_000, 3, 3), dtype=torch.float32, device="cuda:0")
    with pytest.raises(MemoryError, match=str(8 * 200_000 ** 2)):
        CrossDistanceMatrix(x, x).run()


# ---- more tile pairs than one launch takes ---------------------------------------------------
def test_more_tile_pairs_than_a_launch_takes():
    """65,537 x 65,536 frames are 4,097 x 4,096 = 2^24 + 4,096 tile pairs; 2^32 / 256 = 2^24 workgroups is what
    one launch runs in full (a larger grid is not refused: its count wraps), so this is the smallest rectangle
    past the wrap, with a one-frame last tile row.  Five 4-atom structures on a 2^-10 A grid, each frame of A
    and of B one of them moved by a translation on that grid: coordinates, centres (a quotient by 4) and
    deviations are exact, so the deviations of two frames of one structure are the same bits and out[i, j] is a
    function of (state_a[i], state_b[j]) alone -- the 5 x 5 matrix T of the structures against themselves, one
    tile, itself held against numpy f64."""
    import torch

    from rmsf_amd.engine import Engine
    from test_gpu_pairwise import BOUND as SQUARE_BOUND
    from test_gpu_pairwise import reference_sq as square_reference_sq
    n_a, n_b, n_sel, n_states = 65_537, 65_536, 4, 5
    assert (-(-n_a // 16)) * (-(-n_b // 16)) > 2 ** 32 // 256
    need = 48e9   # the 34.4 GB matrix, the 0.5 GB row-block temporaries, and room to spare
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{free / 1e9:.1f} GB of HBM are free, the 65,537 x 65,536 matrix and its check need 48 GB")
    rng = np.random.default_rng(65_537)
    base = (rng.integers(0, 16 * 1024, size=(n_states, n_sel, 3)) / 1024.0).astype(np.float32)
    state_a, state_b = rng.integers(0, n_states, size=n_a), rng.integers(0, n_states, size=n_b)

    def moved(state):
        shift = rng.integers(-8 * 1024, 8 * 1024 + 1, size=(len(state), 1, 3)) / 1024.0
        x = base[state].astype(np.float64) + shift
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x)           # exact in f32
        return x.astype(np.float32)

    xa, xb = moved(state_a), moved(state_b)
    t = engine_cross(base, None, base, None, None, True, cutoff=1e-5)
    sq, s = square_reference_sq(base, None, True)
    ratio = np.abs(t * t - sq) / (SQUARE_BOUND * s)
    print(f"T (5 x 5): max |d2 - d2_ref| / (1e-12 S) = {ratio.max():.3e}")
    assert ratio.max() <= 1.0
    off = ~np.eye(n_states, dtype=bool)
    assert np.sqrt(np.abs(sq[off])).min() > 1.0 and t[off].min() > 1.0     # different structures are far apart
    assert np.all(np.diag(t) == 0.0)

    eng = Engine(torch.device("cuda", 0))
    assert eng.cross_workspace_bytes(n_a, n_b, n_sel) == 0
    ta, tb = torch.tensor(xa, device="cuda:0"), torch.tensor(xb, device="cuda:0")
    ca, ga = eng.pairwise_centres(ta.data_ptr(), ta.stride(0), n_a, n_sel, None, None, True)
    cb, gb = eng.pairwise_centres(tb.data_ptr(), tb.stride(0), n_b, n_sel, None, None, True)
    out = torch.full((n_a + 1, n_b + 1), float("nan"), dtype=torch.float64, device="cuda:0")
    eng.cross_rmsd(ta.data_ptr(), ta.stride(0), n_a, None, ca, ga, tb.data_ptr(), tb.stride(0), n_b, None, cb, gb,
                   n_sel, None, float(n_sel), out, superpose=True, cutoff=1e-5)
    t_dev = torch.tensor(t, device="cuda:0")
    sa_dev, sb_dev = torch.tensor(state_a, device="cuda:0"), torch.tensor(state_b, device="cuda:0")
    for r0 in range(0, n_a, 1024):
        r1 = min(r0 + 1024, n_a)
        assert torch.equal(out[r0:r1, :n_b], t_dev[sa_dev[r0:r1]][:, sb_dev]), f"rows {r0}..{r1 - 1}"
    assert bool(torch.isnan(out[n_a]).all()) and bool(torch.isnan(out[:, n_b]).all())
