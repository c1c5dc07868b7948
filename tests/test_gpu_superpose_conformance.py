"""GPU tier, kernel level: the per-frame transform record (R, COM, rmsd) of
rmsf_superpose / rmsf_superpose_planes / rmsf_superpose_compact against a
high-precision host reference (oracle/superpose_ref.py), at every staging
layout, with and without masses, in each regime of k_frame_stats' balanced
grid -- and every exit of qcp_solve on the device.

A. Plan regimes (T = 32-atom tiles x 64-frame groups, G workgroups):
  (a) one unit per workgroup: selection tails (n_at < 4, counts that are no
      multiple of 4) and frame-group tails (rows clamped to the last frame);
  (b) ranges of 1-2 units: at 330 frames every frame-group seam falls on a
      workgroup boundary, at 394 frames two ranges cross a seam;
  (c) two segments per workgroup (73,605 frames), two or three (76,805):
      the slot advances, k_qcp_frames folds segment indices 1 and 2;
  (d) segments of several tiles: the pipelined step() loop (next tile's
      loads in flight; dense_whole in the compacting kernel).
The plan (T, G, ceil(T/G), P) is restated and asserted per case, and tied to
the library through rmsf_superpose_workspace_bytes, so a retune of the plan's
constants cannot silently move a case into another regime.

Bounds (absolute): COM 1e-9 and R 1e-10 against the QCP oracle as in
test_gpu_kernels.py::test_superpose_vs_oracle; R 1e-8 against the top
eigenvector of K(A) (the QCP-vs-Kabsch bound of tests/test_oracle.py); rmsd
1e-9 against sqrt(2 (E0 - lambda) / N) (rmsd is O(1) A here, the reference's
own rounding ~1e-12); R orthonormal with det +1 to 1e-12; record[13..15] ==
0.  Sensitivity: in every case the reference without the last selected atom
differs from the full one by >= 100 x the rmsd bound in some frame, so the
bound cannot hide an atom lost at a tile tail.

The frames are superposed on a separate reference structure (not a frame of
the batch), so a one-frame batch has a non-zero rmsd too.  Atoms outside the
selection, plane pads and the rows between strided frames are NaN: one read
of them into a sum fails the case.

Measured on MI355X (largest over all cases; every test prints its own with
-s): COM 9.1e-13, rmsd 6.8e-12, R 1.9e-10 against the eigenvector (regime
(c); <= 4e-12 elsewhere) and 8.4e-14 against QCP, orthonormality 2.0e-15.

B. qcp_solve's exits: see test_qcp_batch_every_exit.  Out of scope, and not
asserted anywhere: NEAR-half-turns with noise, where qcprot keeps an
ill-conditioned first candidate (noise of 1e-9 gave a fit error of 1e-4 in
the oracle; that is the reference's behaviour).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import rmsf_oracle as O
from oracle import superpose_ref as SR

pytestmark = pytest.mark.gpu

B_COM, B_RMSD, B_R_EIG, B_R_QCP, B_ORTHO = 1e-9, 1e-9, 1e-8, 1e-10, 1e-12
SENSITIVITY = 100 * B_RMSD

LAYOUTS = ["rows_vec4", "rows_elem", "rows_gather", "planes_vec4", "planes_elem", "planes_gather"]
REGIMES = {
    "a": [(n, f) for n in (3, 4, 5, 31, 32, 33) for f in (1, 63, 65)],
    "b": [(5000, 330), (5000, 394)],
    "c": [(40, 73_605), (40, 76_805)],
    "d": [(25_607, 130)],
}
# regime (b), these layouts: 5000 A added to every coordinate before the f32
# rounding (the kernel's sums are relative to the frame's first selected atom)
SHIFTED = {("b", "rows_vec4"), ("b", "planes_gather")}
# an unsorted selection (the pivot is sel[0], not the lowest index)
UNSORTED = {("a", "rows_gather"), ("b", "rows_gather"), ("c", "planes_gather")}
# frames two frames apart (frame_stride = 2 x frame)
STRIDE2 = {("d", "rows_vec4")}


@pytest.fixture(scope="module")
def eng():
    from rmsf_amd.engine import Engine
    return Engine()


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _dataset(n_sel, nf, shifted):
    """Selected atoms of nf frames (float32 [nf, n_sel, 3]): a structure in a
    100 A box, per-atom noise of 0.2-2 A, a random rigid motion per frame;
    the reference structure (float32 [n_sel, 3]) is another noisy copy;
    masses U[1, 16)."""
    rng = np.random.default_rng(1000 * n_sel + nf)
    base = rng.uniform(0.0, 100.0, (n_sel, 3))
    sigma = rng.uniform(0.2, 2.0, n_sel)
    q = rng.standard_normal((nf, 4))
    rot = SR.quaternion_rotation(q / np.linalg.norm(q, axis=1, keepdims=True))
    x = base + rng.standard_normal((nf, n_sel, 3)) * sigma[:, None] - 50.0
    x = np.einsum("fia,fab->fib", x, rot) + 50.0 + rng.uniform(-5.0, 5.0, (nf, 1, 3))
    ref = base + rng.standard_normal((n_sel, 3)) * sigma[:, None]
    off = 5000.0 if shifted else 0.0
    masses = rng.uniform(1.0, 16.0, n_sel)
    return _ro((x + off).astype(np.float32)), _ro((ref + off).astype(np.float32)), _ro(masses)


@functools.lru_cache(maxsize=None)
def _reference(n_sel, nf, shifted, masses):
    """The host records of a dataset, the QCP oracle's rotations on the
    sampled frames, and the sensitivity figure: computed once, shared by the
    six layouts, never modified."""
    x, ref, m = _dataset(n_sel, nf, shifted)
    m = m if masses else None
    want = SR.records(x, ref, m)
    less = SR.records(x[:, :-1], ref[:-1], None if m is None else m[:-1])
    want["sensitivity"] = float(np.abs(want["rmsd"] - less["rmsd"]).max())
    want["sample"] = SR.sample_frames(nf)
    want["R_qcp"] = SR.oracle_rotations(x, ref, m, want["sample"])
    for v in want.values():
        if isinstance(v, np.ndarray):
            _ro(v)
    return want


def _up4(n):
    return (n + 3) // 4 * 4


def _not4(n):
    return n if n % 4 else n + 1


def _layout(layout, regime, x):
    """Host array of the frames in a staging layout (everything that is not a
    selected coordinate is NaN).  Returns (flat float32 array, offset of the
    first frame in floats, frame stride, plane stride or 0, selection or
    None); the kernel variant each must select is asserted by the caller."""
    nf, n = x.shape[:2]
    rng = np.random.default_rng(n + nf)
    key = (regime, layout)
    sel, ps, off = None, 0, 0
    if layout in ("rows_gather", "planes_gather"):
        n_atoms = n + max(5, n // 4)
        sel = rng.choice(n_atoms, n, replace=False) if key in UNSORTED else np.sort(rng.choice(n_atoms, n, replace=False))
        sel = sel.astype(np.int32)
    if layout == "rows_vec4":
        n_atoms, mult = _up4(n), 2 if key in STRIDE2 else 1
        arr = np.full((nf, mult, n_atoms, 3), np.nan, np.float32)
        arr[:, 0, :n] = x
        fstride = mult * 3 * n_atoms
    elif layout == "rows_elem":
        # (a), (d): frame stride not a multiple of 4 floats; (b): a 16-B
        # stride whose base is one float past a 16-B boundary; (c): both
        n_atoms = _up4(n + 1) if regime == "b" else _not4(n + 1)
        off = 1 if regime in ("b", "c") else 0
        arr = np.full((nf, n_atoms, 3), np.nan, np.float32)
        arr[:, :n] = x
        fstride = 3 * n_atoms
    elif layout == "rows_gather":
        arr = np.full((nf, n_atoms, 3), np.nan, np.float32)
        arr[:, sel] = x
        fstride = 3 * n_atoms
    else:
        if layout == "planes_vec4":
            ps = _up4(n)
        elif layout == "planes_elem":
            ps = _not4(n + 2)  # padded planes
        else:
            ps = n_atoms + 3
        arr = np.full((nf, 3, ps), np.nan, np.float32)
        arr[:, :, (slice(0, n) if sel is None else sel)] = x.transpose(0, 2, 1)
        fstride = 3 * ps
    flat = np.full(off + arr.size, np.nan, np.float32)
    flat[off:] = arr.reshape(-1)
    return flat, off, fstride, ps, sel


def _check_plan(eng, regime, n_sel, nf):
    """The regime's defining properties, from stats_plan() restated; the
    restatement itself is tied to the library by the workspace size (G P
    partials)."""
    p = SR.stats_plan(n_sel, nf)
    assert eng.workspace_bytes(n_sel, nf) == p["G"] * p["P"] * SR.PARTIAL_BYTES, "stats_plan() restatement is stale"
    segs = p["segments"]
    lens = {hi - lo for lo, hi in p["ranges"]}
    if regime == "a":
        assert p["T"] <= 768 and p["G"] == p["T"] and lens == {1}
    elif regime == "b":
        # 330 frames: T = 942 = 6 x 157 and 768 = 6 x 128, so every seam falls
        # on a workgroup boundary and no range crosses one; 394 frames (7
        # groups) leaves two ranges of 2 units across a seam
        assert (p["T"], p["G"], p["len"], p["P"]) == ({330: 942, 394: 1099}[nf], 768, 2, 2) and lens == {1, 2}
        assert sum(len(s) == 2 for s in segs) == {330: 0, 394: 2}[nf], "ranges crossing a frame-group seam"
    elif regime == "c":
        # 73,605 frames: ranges of 3 units over 2-tile groups, so two segments
        # per workgroup (one range of 2 units has one); 76,805 frames: ranges
        # of 4 units that start at a group's second tile have three
        nseg = [len(s) for s in segs]
        if nf == 73_605:
            assert (p["ntiles"], p["T"], p["G"], p["len"], p["P"]) == (2, 2302, 768, 3, 3)
            assert nseg.count(2) == 767 and nseg.count(1) == 1
        else:
            assert (p["ntiles"], p["T"], p["G"], p["len"], p["P"]) == (2, 2402, 768, 4, 3)
            assert set(nseg) == {2, 3} and nseg.count(3) >= 40
    else:
        assert (p["ntiles"], p["ngroups"], p["T"], p["G"], p["len"], p["P"]) == (801, 3, 2403, 768, 4, 2)
        tiles = [t_hi - t_lo for s in segs for _, t_lo, t_hi in s]
        assert max(tiles) >= 3 and np.mean(tiles) > 2.5, "segments of ~3 tiles: the step() loop"
        assert nf - 64 * (p["ngroups"] - 1) == 2
    return p


def _errors(xf, want):
    """Largest deviations of the records xf [F, 16] from the reference."""
    R = xf[:, :9].reshape(-1, 3, 3)
    eye = np.einsum("fab,fcb->fac", R, R) - np.eye(3)
    return dict(
        com=float(np.abs(xf[:, 9:12] - want["com"]).max()),
        rmsd=float(np.abs(xf[:, 12] - want["rmsd"]).max()),
        R_eig=float(np.abs(R - want["R"]).max()),
        R_qcp=float(np.abs(R[want["sample"]] - want["R_qcp"]).max()),
        ortho=float(max(np.abs(eye).max(), np.abs(np.linalg.det(R) - 1.0).max())),
        tail=float(np.abs(xf[:, 13:16]).max()),
    )


def _assert_errors(e, what):
    assert np.isfinite(list(e.values())).all(), (what, e)
    assert e["com"] <= B_COM, (what, e)
    assert e["rmsd"] <= B_RMSD, (what, e)
    assert e["R_eig"] <= B_R_EIG, (what, e)
    assert e["R_qcp"] <= B_R_QCP, (what, e)
    assert e["ortho"] <= B_ORTHO, (what, e)
    assert e["tail"] == 0.0, (what, e)


def _run(eng, dev, off, fstride, ps, sel, ref_h, m_h, nf, n_sel, **dense):
    sdev = eng.sel_tensor(sel)
    mdev = None if m_h is None else torch.tensor(m_h, device=eng.device)
    rdev = torch.tensor(ref_h, device=eng.device)
    ref, info = eng.reference_setup(n_sel, frame_ptr=rdev.data_ptr(), masses=mdev)
    xf = eng.empty(nf, 16)
    xf.fill_(float("nan"))
    work = eng.empty(eng.workspace_bytes(n_sel, nf) // 8 + 1)
    eng.superpose(dev.data_ptr() + 4 * off, fstride, nf, n_sel, sdev, mdev, ref, info, xf, work, pstride=ps, **dense)
    torch.cuda.synchronize()
    return xf.cpu().numpy()


@pytest.mark.parametrize("masses", [False, True], ids=["nomass", "mass"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("regime", list(REGIMES))
def test_records_vs_reference(eng, regime, layout, masses):
    worst, sens = {}, np.inf
    for n_sel, nf in REGIMES[regime]:
        shifted = (regime, layout) in SHIFTED
        x, ref_h, m = _dataset(n_sel, nf, shifted)
        want = _reference(n_sel, nf, shifted, masses)
        assert want["sensitivity"] >= SENSITIVITY, (n_sel, nf, want["sensitivity"])
        sens = min(sens, want["sensitivity"])
        _check_plan(eng, regime, n_sel, nf)
        flat, off, fstride, ps, sel = _layout(layout, regime, x)
        dev = torch.tensor(flat, device=eng.device)
        # the staging path this layout must select (superpose_impl's test)
        vec4 = sel is None and fstride % 4 == 0 and ps % 4 == 0 and (dev.data_ptr() + 4 * off) % 16 == 0
        assert vec4 == layout.endswith("vec4") and (sel is not None) == layout.endswith("gather")
        xf = _run(eng, dev, off, fstride, ps, sel, ref_h, m if masses else None, nf, n_sel)
        e = _errors(xf, want)
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
        _assert_errors(e, (regime, layout, masses, n_sel, nf))
    print(f"\n  ({regime}) {layout:13s} {'mass  ' if masses else 'nomass'} " +
          " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" | sensitivity {sens:.1e}")


@pytest.mark.parametrize("masses", [False, True], ids=["nomass", "mass"])
def test_compact_multi_tile_segments(eng, masses):
    """rmsf_superpose_compact in regime (d): whole tiles with a successor in
    one segment (dense_whole between the next tile's loads and the sums), at
    a packed pitch (3 x 25,607: odd, float stores), a 16-B pitch (float4
    stores) and a pitch of 2 mod 4.  Records bit for bit those of
    rmsf_superpose, themselves within the bounds of the reference; the copy
    equals the selected rows exactly and nothing else is written."""
    (n_sel, nf), = REGIMES["d"]
    x, ref_h, m = _dataset(n_sel, nf, False)
    want = _reference(n_sel, nf, False, masses)
    assert want["sensitivity"] >= SENSITIVITY
    _check_plan(eng, "d", n_sel, nf)
    flat, off, fstride, ps, sel = _layout("rows_gather", "d", x)
    dev = torch.tensor(flat, device=eng.device)
    mh = m if masses else None
    xf0 = _run(eng, dev, off, fstride, ps, sel, ref_h, mh, nf, n_sel)
    e = _errors(xf0, want)
    _assert_errors(e, ("compact", masses))
    for dstride in (3 * n_sel, _up4(3 * n_sel), 3 * n_sel + 5):
        dense = torch.full((nf + 1, dstride), float("nan"), dtype=torch.float32, device=eng.device)
        xf1 = _run(eng, dev, off, fstride, ps, sel, ref_h, mh, nf, n_sel, dense_out=dense.data_ptr(),
                   dense_stride=dstride)
        np.testing.assert_array_equal(xf1.view(np.uint64), xf0.view(np.uint64), err_msg=f"records, pitch {dstride}")
        d = dense.cpu().numpy()
        np.testing.assert_array_equal(d[:nf, :3 * n_sel].view(np.uint32), x.reshape(nf, -1).view(np.uint32))
        assert np.isnan(d[:nf, 3 * n_sel:]).all() and np.isnan(d[nf]).all()
    print(f"\n  compact (d) {'mass  ' if masses else 'nomass'} " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))


# ---------------------------------------------------------------------------
# B. every exit of qcp_solve


# R of the perturbed half-turns against the QCP oracle.  qcp_solve and the
# oracle are the same sequence of IEEE double +, -, *, /, sqrt (the library is
# built without contraction), so they agree to the last bit; 8 ulp of 1 is
# allowed.  At the margin the branch condition demands (vanishing candidates
# <= 1e-9), a cofactor term that is 0 at the exact half-turn carries only
# 1e-14..1e-11 of R, below the 1e-13 of the other cases: flipping each of the
# 48 terms' signs in the oracle moves R by more than this bound for 47 of them
# (by more than 1e-13 for 40).  The 48th, -a31 a1223_1322 in the fourth
# candidate's q4, is a product of two factors that both vanish at q = (0, 0,
# 0, 1): below an ulp on every input that reaches that candidate.
B_NEAR = 8 * np.finfo(np.float64).eps


def _half_turn(axis):
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    return 2.0 * np.outer(u, u) - np.eye(3)


def _generic_rotation(rng):
    q = rng.standard_normal(4)
    return SR.quaternion_rotation(q / np.linalg.norm(q))


def _qcp_cases():
    """name -> (ref, mob, expected exit 1-4 or 0 = identity, exact fit?, bound
    on the vanishing candidates) at N = 40 atoms, coordinates ~N(0, 1) A.  A
    half-turn has q1 = 0, so the first candidate vanishes; about an axis in
    the yz plane q2 = 0 too, about z only q4 is left.
    The identity exit at 0.02 A: the candidates' norms^2 are (the product of
    K's three eigenvalue gaps)^2 q_k^2 ~ (8 (2 N s^2)^3)^2 = 7e-8 at N = 40,
    s = 0.02 -- below evecprec = 1e-6 by a factor of 10, not of 1e3 (rounding
    moves them by ~1e-20, so the branch is no coin toss either way).  The
    same structure at 0.01 A (norms^2 scale with s^12) has the full margin."""
    rng = np.random.default_rng(77)

    def ref():
        r = rng.standard_normal((40, 3))
        return r - r.mean(0)

    cases = {}
    for name, axis, col in (("column2", (1, 2, 3), 2), ("column3", (0, 1, 2), 3), ("column4", (0, 0, 1), 4),
                            ("half_turn_x", (1, 0, 0), 2)):
        r = ref()
        cases[name] = (r, r @ _half_turn(axis), col, True, 1e-9)
    # An exact half-turn leaves the taken candidate's other components at
    # exactly 0 term by term (about z: q = (0, 0, 0, 1), and a34 = a13 = 0),
    # so a wrong sign in one of their cofactor terms would go unseen.  The
    # same half-turns followed by a generic rotation of 5e-12 rad: the earlier
    # candidates stay below 1e-9 (their norms are ~5e-12 x the gaps' product
    # of ~4e6), the branch is the same, and every term of the taken candidate
    # is a part of the result again (B_NEAR).
    w = np.array([0.3, -0.5, 0.8]) * 5e-12 / np.linalg.norm([0.3, -0.5, 0.8])
    tiny = np.eye(3) + np.array([[0, w[2], -w[1]], [-w[2], 0, w[0]], [w[1], -w[0], 0]])
    for name, axis, col in (("column2_near", (1, 2, 3), 2), ("column3_near", (0, 1, 2), 3),
                            ("column4_near", (0, 0, 1), 4)):
        r = ref()
        cases[name] = (r, r @ _half_turn(axis) @ tiny, col, True, 1e-9)
    r = ref()
    cases["identity_fit"] = (r, r.copy(), 1, True, 1e-9)
    r = ref()
    cases["reflected"] = (r, r * np.array([1.0, 1.0, -1.0]), 1, False, 1e-9)
    r = ref()
    mob = r @ _generic_rotation(rng) + 0.1 * rng.standard_normal((40, 3))
    mob -= mob.mean(0)
    cases["identity_exit_0.02"] = (0.02 * r, 0.02 * mob, 0, False, 1e-7)
    cases["identity_exit_0.01"] = (0.01 * r, 0.01 * mob, 0, False, 1e-9)
    return cases


def _check_branch(A, expect, what, vanish_bound=1e-9):
    """The condition on the inputs: candidates meant to vanish <= 1e-9, the
    one taken >= 1e-3 -- a margin of 1e3 on each side of evecprec = 1e-6."""
    got, n2 = SR.qcp_exit(A)
    assert got == expect, (what, got, n2)
    vanish = n2 if expect == 0 else n2[:expect - 1]
    assert (vanish <= vanish_bound).all(), (what, n2)
    if expect:
        assert n2[expect - 1] >= 1e-3, (what, n2)


def test_qcp_batch_every_exit(eng):
    """rmsf_qcp_batch through each of qcp_solve's five exits: the four
    candidate quaternions (rows of the adjugate of K - lambda I; exact
    half-turns make the earlier ones vanish) and the identity (a 0.02 A
    structure: all four below 1e-6), plus a half-turn about x, the identity
    fit, a reflected structure and the half-turns a 5e-12 rad rotation off
    (see _qcp_cases), placed among 250 generic fits so they sit at varied
    lanes of the waves.  R 1e-13 and rmsd 1e-11 against the QCP
    oracle (the bounds of test_qcp_batch_vs_oracle); |mob R - ref| <= 1e-8
    for the exact fits, which does not depend on the oracle's QCP."""
    rng = np.random.default_rng(78)
    cases = _qcp_cases()
    where = dict(zip(cases, (0, 37, 63, 64, 130, 191, 256, 257, 100, 5, 75, 222)))
    assert len(where) == len(cases)
    n_total = 250 + len(cases)
    assert max(where.values()) < n_total
    slots = {v: k for k, v in where.items()}
    items = []
    for i in range(n_total):
        if i in slots:
            items.append((slots[i],) + cases[slots[i]])
        else:
            r = rng.standard_normal((40, 3))
            mob = r @ _generic_rotation(rng) + 0.3 * rng.standard_normal((40, 3))
            items.append(("generic", r - r.mean(0), mob - mob.mean(0), 1, False, 1e-9))
    As, E0s, exp = [], [], []
    for name, r, mob, col, _, vanish in items:
        A, E0 = O.inner_product(r, mob)
        _check_branch(A, col, name, vanish)
        As.append(A)
        E0s.append(E0)
        exp.append(O.fast_calc_rmsd_and_rotation(A, E0, 40.0))
    dev = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=eng.device)
    rot, rmsd = eng.qcp_batch(dev(As), dev(E0s), dev(np.full(n_total, 40.0)))
    torch.cuda.synchronize()
    rot, rmsd = rot.cpu().numpy().reshape(-1, 3, 3), rmsd.cpu().numpy()
    want_R = np.array([e[0] for e in exp]).reshape(-1, 3, 3)
    want_rmsd = np.array([e[1] for e in exp])
    line = []
    for i, (name, r, mob, col, exact, _) in enumerate(items):
        if name == "generic":
            continue
        eR, er = np.abs(rot[i] - want_R[i]).max(), abs(rmsd[i] - want_rmsd[i])
        fit = np.abs(mob @ rot[i] - r).max() if exact else float("nan")
        line.append(f"{name}: R {eR:.1e} rmsd {er:.1e} fit {fit:.1e}")
        assert eR <= (B_NEAR if name.endswith("_near") else 1e-13) and er <= 1e-11, (name, eR, er)
        assert abs(np.linalg.det(rot[i]) - 1.0) <= 1e-12, name
        if exact:
            assert fit <= 1e-8, (name, fit)
        if col == 0:
            assert np.array_equal(rot[i], np.eye(3)), name
            assert want_rmsd[i] > 1e-4  # a real misfit, not 0 = 0
    np.testing.assert_allclose(rot, want_R, rtol=0, atol=1e-13)
    np.testing.assert_allclose(rmsd, want_rmsd, rtol=0, atol=1e-11)
    print("\n  " + "\n  ".join(line) + f"\n  all {n_total}: R {np.abs(rot - want_R).max():.1e} "
          f"rmsd {np.abs(rmsd - want_rmsd).max():.1e}")


@functools.lru_cache(maxsize=None)
def _half_turn_frames(n_sel):
    """9 frames: 0 the reference; 1-4 its half-turns about x, y, z and
    (1,1,0)/sqrt(2) -- sign flips and an x <-> y swap, exact in float32; 5
    the reference again; 6-8 generic.  The coordinate scale keeps N sigma^2
    = 40-256, where the vanishing candidates' rounding noise (~eps (N
    sigma^2)^3, squared) stays far below evecprec."""
    rng = np.random.default_rng(n_sel)
    s = 1.0 if n_sel <= 40 else 0.25
    f0 = (s * (rng.standard_normal((n_sel, 3)) + np.array([3.0, -2.0, 1.0]))).astype(np.float32)
    x = np.empty((9, n_sel, 3), np.float32)
    x[0] = x[5] = f0
    x[1] = f0 * np.array([1, -1, -1], np.float32)
    x[2] = f0 * np.array([-1, 1, -1], np.float32)
    x[3] = f0 * np.array([-1, -1, 1], np.float32)
    x[4] = f0[:, [1, 0, 2]] * np.array([1, 1, -1], np.float32)
    for f in (6, 7, 8):
        x[f] = ((f0.astype(np.float64) + 0.3 * s * rng.standard_normal((n_sel, 3))) @ _generic_rotation(rng)
                + s * rng.uniform(-2, 2, 3)).astype(np.float32)
    return _ro(x)


@pytest.mark.parametrize("n_sel", [40, 4096])
def test_superpose_half_turn_frames(eng, n_sel):
    """The fallback candidates through rmsf_superpose (k_frame_stats'
    sums feeding qcp_solve): exact half-turns of the reference about x, y
    (candidates 2 and 3), z (4) and (1,1,0)/sqrt(2) (2), and the reference
    itself (1), among generic frames."""
    x = _half_turn_frames(n_sel)
    want = SR.records(x, x[0])
    for f, col in enumerate((1, 2, 3, 4, 2, 1, 1, 1, 1)):
        _check_branch(want["A"][f], col, (n_sel, f))
    which = np.arange(9)
    want["sample"], want["R_qcp"] = which, SR.oracle_rotations(x, x[0], None, which)
    dev = torch.tensor(x, device=eng.device)
    xf = _run(eng, dev, 0, 3 * n_sel, 0, None, x[0], None, 9, n_sel)
    e = _errors(xf, want)
    # Frames 0-5 fit exactly: lambda = E0 = (G_ref + G_mob) / 2 in exact
    # arithmetic, and rmsd^2 = 2 |E0 - lambda| / N is what rounding leaves of
    # that difference.  E0 and lambda each carry a relative error of a few
    # eps (the f64 sums of N terms, the Newton iteration's last step), so
    # |E0 - lambda| <= 32 eps (G_ref + G_mob), i.e. rmsd^2 <= 64 eps (G_ref +
    # G_mob) / N.
    eps = np.finfo(np.float64).eps
    bound2 = 64 * eps * (want["g_ref"] + want["g_mob"][:6]) / n_sel
    ratio = float((xf[:6, 12] ** 2 / bound2).max())
    print(f"\n  half-turn frames n_sel {n_sel}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items() if k != "rmsd") +
          f" rmsd(6-8) {np.abs(xf[6:, 12] - want['rmsd'][6:]).max():.2e} exact-fit rmsd^2/bound {ratio:.2e}")
    assert (xf[:6, 12] ** 2 <= bound2).all(), (xf[:6, 12], np.sqrt(bound2))
    assert np.abs(xf[6:, 12] - want["rmsd"][6:]).max() <= B_RMSD
    e["rmsd"] = 0.0  # asserted above, frames 0-5 by the rounding bound
    _assert_errors(e, ("half-turn frames", n_sel))
