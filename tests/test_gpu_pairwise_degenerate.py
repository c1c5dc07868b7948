"""GPU tier: the RMSD-matrix kernels (csrc/pairwise.hip) where the largest
root of the QCP quartic is not simple, and on non-finite frames.

Data: tests/pairwise_zoo.py -- a generic frame and its point reflection,
nested cubes (s0 = s1 = s2) and their rotated reflections with noise 0, 1e-6,
1e-4, 1e-2 A, atoms on a line and rotated copies of it (scaled, with noise
1e-5, 1e-3, 1e-1 A), a planar frame, a rotated copy and its mirror image, a
collapsed frame, two all-zero frames; frames of 1 and 2 atoms at engine level.
The test proves its own data degenerate: from the key matrix of each flagged
pair, computed in numpy, the two largest eigenvalues differ by at most 1e-4 of
the largest.

Reference and bound are those of tests/test_gpu_pairwise.py and
tests/test_gpu_cross_rmsd.py, unchanged: numpy's SVD in f64, ``|d^2_gpu -
d^2_ref| <= 1e-12 S_ij``.  Every off-diagonal pair is compared, duplicates
included, at ``cutoff = 0`` so that the cutoff hides nothing.  Newton's
iteration alone misses this bound on the flagged pairs by up to 4e6 times
(tests/test_pair_lambda_host.py asserts that on the host); the epilogue takes
the largest eigenvalue of the key matrix by Jacobi there.

Shapes: (20, 8) is the direct plan with two frame tiles (a diagonal tile, an
off-diagonal one with its mirrored store, a partial one); (17, 40) is split-K,
the epilogue in ``k_pw_fold``; (20, 17, 8) and (5, 17, 40) the same for the
rectangle.

Non-finite frames, at (20, 33) and (20, 17, 33) -- partial tiles, one atom
past a stage: a NaN or +Inf in the last frame (which lanes past the last frame
read too), a middle frame, the last selected atom (which lanes past the range
read too) makes that frame's row and column NaN and changes no other bit; in an
atom that is not selected it changes nothing.  (Without superposition an atom
at +Inf is +Inf or NaN away: G_i - 2 tr A_ij is inf + inf or inf - inf.)  For the
rectangle ``nearest`` / ``nearest_dist`` are numpy.argmin's: the first NaN.

The largest ratios to the bound measured on an MI355X are in DESIGN section 4,
"Degenerate pairs".
"""
import functools

import numpy as np
import pytest

import pairwise_zoo as Z
from test_gpu_cross_rmsd import engine_cross
from test_gpu_cross_rmsd import reference_sq as cross_reference_sq
from test_gpu_pairwise import BOUND, make_traj, reference_sq, same_bits

pytestmark = pytest.mark.gpu


# ---- running the kernels ------------------------------------------------------------------
def engine_square(x, sel, w, superpose, cutoff=0.0):
    """rmsf_pairwise_rmsd on the host array x [F, n_atoms, 3] copied to HBM."""
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    n_frames = len(x)
    n_sel = x.shape[1] if sel is None else len(sel)
    t = torch.tensor(x, device="cuda:0")
    sel_dev = eng.sel_tensor(sel)
    w_dev = None if w is None else torch.tensor(w, device="cuda:0")
    w_total = float(n_sel) if w is None else float(w.sum())
    centre, g = eng.pairwise_centres(t.data_ptr(), t.stride(0), n_frames, n_sel, sel_dev, w_dev, superpose)
    need = eng.pairwise_workspace_bytes(n_frames, n_sel)
    work = eng.empty(need // 8) if need else None
    out = torch.full((n_frames, n_frames), float("nan"), dtype=torch.float64, device="cuda:0")
    eng.pairwise_rmsd(t.data_ptr(), t.stride(0), n_frames, n_sel, sel_dev, w_dev, w_total, centre, g, out,
                      superpose=superpose, cutoff=cutoff, work=work)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def workspace_bytes(n_frames, n_sel, n_b=None):
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    return eng.pairwise_workspace_bytes(n_frames, n_sel) if n_b is None else \
        eng.cross_workspace_bytes(n_frames, n_b, n_sel)


def rows(x, sel):
    return x if sel is None else x[:, sel]


@functools.lru_cache(maxsize=None)
def square_reference(kind, n_frames, n_sel, gathered, weighted, superpose):
    x = (Z.zoo if kind == "zoo" else Z.few_atoms)(n_frames, n_sel, gathered)
    sq, s = reference_sq(rows(x, Z.selection(n_sel, gathered)), Z.weights_of(n_sel) if weighted else None, superpose)
    sq.setflags(write=False)
    s.setflags(write=False)
    return sq, s


def cross_sides(f_a, f_b, n_sel, gathered):
    """A: the zoo of f_a frames; B: the zoo of f_b frames with rotations,
    noise and translations of its own."""
    return Z.zoo(f_a, n_sel, gathered), Z.zoo(f_b, n_sel, gathered, seed=1)


@functools.lru_cache(maxsize=None)
def cross_reference(f_a, f_b, n_sel, gathered, weighted, superpose):
    a, b = cross_sides(f_a, f_b, n_sel, gathered)
    sel = Z.selection(n_sel, gathered)
    sq, s = cross_reference_sq(rows(a, sel), rows(b, sel), Z.weights_of(n_sel) if weighted else None, superpose)
    sq.setflags(write=False)
    s.setflags(write=False)
    return sq, s


def check(m, sq_ref, s_scale, keep, n_expected, label, names=None) -> float:
    """No NaN, every kept pair inside the bound (asserted as |d^2 - d^2_ref|
    <= 1e-12 S, which also holds pairs with S = 0 to exactly 0); returns and
    prints the largest ratio, and the pair that has it."""
    assert m.shape == sq_ref.shape and m.dtype == np.float64
    assert not np.isnan(m).any(), f"{label}: NaN in the matrix"
    assert keep.sum() == n_expected, f"{label}: {keep.sum()} pairs compared, not {n_expected}"
    err = np.abs(m * m - sq_ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / (BOUND * s_scale))
    ratio = np.where(keep, ratio, 0.0)
    i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    who = f" at ({names[0][i]}, {names[1][j]})" if names else f" at ({i}, {j})"
    print(f"{label}: max |d2 - d2_ref| / (1e-12 S) = {ratio[i, j]:.3e}{who}")
    assert np.all(err[keep] <= BOUND * s_scale[keep]), f"{label}: ratio {ratio[i, j]}{who}"
    return float(ratio[i, j])


def check_symmetric(m):
    assert same_bits(m, np.ascontiguousarray(m.T)), "D != D.T"
    assert not m.diagonal().any(), "the diagonal is exactly zero"


def family_ratios(m, sq_ref, s_scale, order_a, order_b, label):
    """The largest ratio of each flagged family (printed: DESIGN's table)."""
    err = np.abs(m * m - sq_ref)
    for family, first, others in Z.FLAGGED:
        if first not in order_a:
            continue
        i = order_a.index(first)
        js = [order_b.index(o) for o in others if o in order_b]
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err[i, js] == 0.0, 0.0, err[i, js] / (BOUND * s_scale[i, js]))
        print(f"{label} family {family}: max ratio {r.max():.3e}")


def assert_flagged_degenerate(xa, xb, order_a, order_b, w, label):
    """The flagged pairs of the selected rows xa, xb are degenerate: the test
    cannot quietly turn generic."""
    a, _, _ = Z.pair_inputs(xa, xb, w)
    seen = 0
    for family, first, others in Z.FLAGGED:
        if first not in order_a:
            continue
        i = order_a.index(first)
        js = [order_b.index(o) for o in others if o in order_b]
        assert js, family
        Z.assert_degenerate(a[i, js], f"{label} {family}")
        seen += 1
    assert seen >= 4, f"{label}: only {seen} flagged families in this shape"


# ---- 1. the square matrix on the zoo ---------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("n_frames,n_sel,split", [(20, 8, False), (17, 40, True)], ids=["direct-20x8", "splitk-17x40"])
def test_square_zoo(n_frames, n_sel, split, gathered, weighted):
    import torch

    from rmsf_amd import DistanceMatrix
    assert (workspace_bytes(n_frames, n_sel) > 0) == split          # the epilogue runs in k_pw_fold / k_pw_tiles
    x, sel = Z.zoo(n_frames, n_sel, gathered), Z.selection(n_sel, gathered)
    w = Z.weights_of(n_sel) if weighted else None
    order = Z.ORDER[n_frames]
    label = f"square ({n_frames} x {n_sel}) gathered={gathered} weighted={weighted}"
    assert_flagged_degenerate(rows(x, sel), rows(x, sel), order, order, w, label)
    off = ~np.eye(n_frames, dtype=bool)

    sq_ref, s = square_reference("zoo", n_frames, n_sel, gathered, weighted, True)
    m = engine_square(x, sel, w, True)
    check_symmetric(m)
    check(m, sq_ref, s, off, n_frames * n_frames - n_frames, label, (order, order))
    family_ratios(m, sq_ref, s, order, order, label)
    z0, z1 = order.index("Z0"), order.index("Z1")
    assert m[z0, z1] == 0.0 and m[z1, z0] == 0.0, "the two all-zero frames are not at exactly 0"
    assert same_bits(m, engine_square(x, sel, w, True)), "two runs differ in their bits"

    # no Newton step without superposition: the control
    sq_plain, s_plain = square_reference("zoo", n_frames, n_sel, gathered, weighted, False)
    p = engine_square(x, sel, w, False)
    check_symmetric(p)
    check(p, sq_plain, s_plain, off, n_frames * n_frames - n_frames, label + " plain", (order, order))

    # DistanceMatrix: the engine's bits; at the default cutoff the same but for the pairs it zeroes
    dev = torch.tensor(x, device="cuda:0")
    r = DistanceMatrix(dev, select=sel, weights=w, cutoff=0.0).run().results.dist_matrix
    assert same_bits(r, m), "DistanceMatrix and the engine differ in their bits"
    r = DistanceMatrix(dev, select=sel, weights=w).run().results.dist_matrix
    cut = m <= 1e-5
    assert cut[z0, z1] and not r[cut].any() and same_bits(r[~cut], m[~cut])
    check(r, sq_ref, s, off & ~cut, n_frames * n_frames - n_frames - int((off & cut).sum()),
          label + " DistanceMatrix", (order, order))


# ---- 2. the rectangle on the zoo -----------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("f_a,f_b,n_sel,split", [(20, 17, 8, False), (5, 17, 40, True)],
                         ids=["direct-20x17x8", "splitk-5x17x40"])
def test_cross_zoo(f_a, f_b, n_sel, split, gathered, weighted):
    import torch

    from rmsf_amd import CrossDistanceMatrix
    assert (workspace_bytes(f_a, n_sel, f_b) > 0) == split
    (a, b), sel = cross_sides(f_a, f_b, n_sel, gathered), Z.selection(n_sel, gathered)
    w = Z.weights_of(n_sel) if weighted else None
    oa, ob = Z.ORDER[f_a], Z.ORDER[f_b]
    label = f"cross ({f_a} x {f_b} x {n_sel}) gathered={gathered} weighted={weighted}"
    assert_flagged_degenerate(rows(a, sel), rows(b, sel), oa, ob, w, label)
    every = np.ones((f_a, f_b), dtype=bool)

    sq_ref, s = cross_reference(f_a, f_b, n_sel, gathered, weighted, True)
    m = engine_cross(a, sel, b, sel, w, True, cutoff=0.0)
    check(m, sq_ref, s, every, f_a * f_b, label, (oa, ob))
    family_ratios(m, sq_ref, s, oa, ob, label)
    for zb in ("Z0", "Z1"):
        assert m[oa.index("Z0"), ob.index(zb)] == 0.0, "two all-zero frames are not at exactly 0"
    assert same_bits(m, engine_cross(a, sel, b, sel, w, True, cutoff=0.0)), "two runs differ in their bits"

    sq_plain, s_plain = cross_reference(f_a, f_b, n_sel, gathered, weighted, False)
    p = engine_cross(a, sel, b, sel, w, False, cutoff=0.0)
    check(p, sq_plain, s_plain, every, f_a * f_b, label + " plain", (oa, ob))

    ta, tb = torch.tensor(a, device="cuda:0"), torch.tensor(b, device="cuda:0")
    r = CrossDistanceMatrix(ta, tb, select=sel, weights=w, cutoff=0.0).run().results
    assert same_bits(r.dist_matrix, m), "CrossDistanceMatrix and the engine differ in their bits"
    np.testing.assert_array_equal(r.nearest, np.argmin(m, axis=1))
    assert same_bits(r.nearest_dist, m.min(axis=1))
    r = CrossDistanceMatrix(ta, tb, select=sel, weights=w).run().results.dist_matrix
    cut = m <= 1e-5
    assert cut.any() and not r[cut].any() and same_bits(r[~cut], m[~cut])
    check(r, sq_ref, s, ~cut, f_a * f_b - int(cut.sum()), label + " CrossDistanceMatrix", (oa, ob))


# ---- 3. one and two atoms, engine level (the public classes refuse fewer than 3) -----------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("n_sel", [1, 2])
def test_one_and_two_atoms(n_sel, gathered, weighted):
    n_frames = 17
    x, sel = Z.few_atoms(n_frames, n_sel, gathered), Z.selection(n_sel, gathered)
    w = Z.weights_of(n_sel) if weighted else None
    label = f"({n_frames} x {n_sel}) gathered={gathered} weighted={weighted}"
    off = ~np.eye(n_frames, dtype=bool)
    a, e0, _ = Z.pair_inputs(rows(x, sel), rows(x, sel), w)
    Z.assert_degenerate(a[off], label)                       # rank 1 (two atoms) or 0 (one)
    if n_sel == 1:
        assert not e0.any() and not a.any()                  # a frame of one atom is its own centre exactly
    # (one atom without superposition: S = 0 for every pair, and the distance of
    # two arbitrary points is not computed exactly)
    for superpose in (True, False) if n_sel == 2 else (True,):
        sq_ref, s = square_reference("few", n_frames, n_sel, gathered, weighted, superpose)
        m = engine_square(x, sel, w, superpose)
        check_symmetric(m)
        check(m, sq_ref, s, off, n_frames * n_frames - n_frames, f"{label} superpose={superpose}")
        assert same_bits(m, engine_square(x, sel, w, superpose))
        if n_sel == 1 and superpose:
            assert not m.any(), "one atom superposes on one atom: every distance is exactly 0"
        # the rectangle of the same frames, B turned round
        xb = np.ascontiguousarray(x[::-1])
        sq_c, s_c = cross_reference_sq(rows(x, sel), rows(xb, sel), w, superpose)
        c = engine_cross(x, sel, xb, sel, w, superpose, cutoff=0.0)
        check(c, sq_c, s_c, np.ones_like(c, dtype=bool), n_frames * n_frames, f"cross {label} superpose={superpose}")


# ---- 4. non-finite frames stay in their own row and column ------------------------------------------
NF, NB, NSEL = 20, 17, 33


def poison_sites(gathered):
    """(name, frame, atom row of the frame, coordinate)."""
    last_sel = 3 * NSEL - 2 if gathered else NSEL - 1
    mid_sel = 3 * 10 + 1 if gathered else 10
    sites = [("last frame", NF - 1, mid_sel, 1), ("middle frame", 7, mid_sel, 2), ("last selected atom", 3, last_sel, 0)]
    if gathered:
        sites += [("atom not selected", 5, 0, 1), ("atom after the last selected", NF - 1, 3 * NSEL - 1, 2)]
    return sites


def poisoned(x, frame, atom, coord, v):
    y = x.copy()
    y[frame, atom, coord] = v
    return y


def assert_only_row_and_column(m, clean, frame, axes, label, nan=True):
    """m is NaN along `frame` of each of `axes` (but a square matrix' diagonal,
    the 0 always written) and equal to `clean` in its bits elsewhere.  Not
    `nan`: +Inf will do -- an atom at infinity, without superposition, is
    infinitely far (G_i - 2 tr A_ij is inf + inf or inf - inf by the sign of the
    other frame's deviation)."""
    hit = np.zeros(m.shape, dtype=bool)
    if 0 in axes:
        hit[frame, :] = True
    if 1 in axes:
        hit[:, frame] = True
    if axes == (0, 1):
        assert m[frame, frame] == 0.0, label
        hit[frame, frame] = False
    assert (np.isnan(m[hit]) | (not nan and np.isposinf(m[hit]))).all(), \
        f"{label}: a pair of the non-finite frame is not NaN"
    assert not np.isnan(m[~hit]).any(), f"{label}: the non-finite frame leaked"
    assert same_bits(m[~hit], clean[~hit]), f"{label}: another entry changed"


@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
def test_non_finite_frames_square(gathered, superpose):
    n_atoms = 3 * NSEL if gathered else NSEL
    x, sel = make_traj(n_atoms, NF), Z.selection(NSEL, gathered)
    clean = engine_square(x, sel, None, superpose)
    assert not np.isnan(clean).any()
    for name, frame, atom, coord in poison_sites(gathered):
        for v in (np.nan, np.inf):
            m = engine_square(poisoned(x, frame, atom, coord, v), sel, None, superpose)
            label = f"{v} in {name} gathered={gathered} superpose={superpose}"
            if sel is not None and atom not in sel:
                assert same_bits(m, clean), f"{label}: an atom outside the selection changed the matrix"
            else:
                assert_only_row_and_column(m, clean, frame, (0, 1), label, nan=superpose or np.isnan(v))


@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
def test_non_finite_frames_cross(gathered, superpose):
    import torch

    from rmsf_amd import CrossDistanceMatrix
    n_atoms = 3 * NSEL if gathered else NSEL
    x, sel = make_traj(n_atoms, NF + NB), Z.selection(NSEL, gathered)
    a, b = x[:NF], x[NF:]
    clean = engine_cross(a, sel, b, sel, None, superpose, cutoff=0.0)
    assert not np.isnan(clean).any()
    for name, frame, atom, coord in poison_sites(gathered):
        selected = sel is None or atom in sel
        for v in (np.nan, np.inf):
            for side in ("A", "B"):
                fr = frame if side == "A" or frame != NF - 1 else NB - 1          # B's last frame
                pa = poisoned(a, fr, atom, coord, v) if side == "A" else a
                pb = poisoned(b, fr, atom, coord, v) if side == "B" else b
                label = f"{v} in {name} of {side} gathered={gathered} superpose={superpose}"
                m = engine_cross(pa, sel, pb, sel, None, superpose, cutoff=0.0)
                if not selected:
                    assert same_bits(m, clean), f"{label}: an atom outside the selection changed the matrix"
                else:
                    assert_only_row_and_column(m, clean, fr, (0,) if side == "A" else (1,), label,
                                               nan=superpose or np.isnan(v))
                if not superpose:
                    continue
                # nearest follows numpy.argmin: a NaN is the least, the first NaN is named
                r = CrossDistanceMatrix(torch.tensor(pa, device="cuda:0"), torch.tensor(pb, device="cuda:0"),
                                        select=sel, cutoff=0.0).run().results
                assert same_bits(r.dist_matrix, m), label
                np.testing.assert_array_equal(r.nearest, np.argmin(m, axis=1), err_msg=label)
                assert same_bits(r.nearest_dist, m[np.arange(NF), r.nearest]), label
                if selected:
                    if side == "B":
                        assert np.all(r.nearest == fr) and np.isnan(r.nearest_dist).all(), label
                    else:
                        assert r.nearest[fr] == 0 and np.isnan(r.nearest_dist[fr]), label
                        assert not np.isnan(np.delete(r.nearest_dist, fr)).any(), label
