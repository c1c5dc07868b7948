"""GPU tier: the serial chains of ``exact=True`` (wave_seq_sum, pc_seq_sum and
chain_block in csrc/rmsf_kernels.hip) at their own block edges, against a
sequential numpy sum of the same terms, bit for bit.

Every shape comes from rmsf_internal_seq_chain_layout -- the atoms per group
(g) and per block (B) of the chain, the chain counts up to which a launch
runs two-wave chains (P) and one-wave chains with reserved LDS (R), and the
atom count from which the reference's fill and centring run grid-wide (G) --
so a change of the kernel's block moves the tests with it.

"Sequential" is ``np.cumsum(terms)[-1]`` (the oracle's _seq_sum): one add
per term, in order.  (cumsum starts from the first term where the kernel's
chain starts from +0.0; they differ only when every term is -0.0, which this
generator does not produce.)  The terms are formed with the rounding of the
kernel's ``term`` lambda, one numpy operation per C operation.  What is
compared are the raw sums a chain writes -- the frames' COMs, the record's
A[0..8] and G1 before the QCP, the reference record's COM, sum r and G2 --
not a result derived from them.

What an equal sum proves depends on the inputs.  A dropped, duplicated or
mis-padded term moves a sum in its leading digits.  A wrong ORDER is seen only
where the rounding differs: for every case of more than two blocks the test
asserts, on the reference alone, that summing the same terms block by block
(each block from +0.0, the partials added in order) gives other bits than the
sequential sum in at least half of the case's chains (``_order_share``;
measured: 86-100 % of the frames' chains, 6 or 7 of the reference record's
7, and 2-4 of the 4 left to an unweighted reference frame).  The chains of an
unweighted COM of f32 coordinates are left out of that count and nothing is
claimed for them: their terms are f32 values times 1.0, whose sum is exact
in f64 in any order, so no input can tell.  A
swap of two neighbouring terms changes only 1-7 of 144 such chains and is
NOT claimed to be caught.

Chains in which the block-by-block sum differs (contiguous / gathered):
      n      COM, 5 frames   InnerProduct, 5   COM, 257 frames   InnerProduct, 77
    2 B + 1  15 / 14 of 15   48 / 47 of 50     747 / 739 of 771  731 / 735 of 770
    3 B      13 / 14         45 / 46
    3 B + 1  13 / 14         45 / 48
    4 B      15 / 15         48 / 48
    4 B + 1  15 / 15         50 / 48           738 / 747         741 / 738
  the reference record, 2 B + 1 ... G + B + 1: 7 of 7 from sweep-1 sums and
  from a weighted frame (6 of 7 gathered at 3 B and 3 B + 1); unweighted
  frame 4 of 4, but 2 / 3 at 3 B and 3 / 2 at 4 B."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import rmsf_oracle as O
from oracle import synth as SY

pytestmark = pytest.mark.gpu


def chain_layout():
    """(g, B, P, R, G) as the kernel was built."""
    from rmsf_amd import _lib
    fn = _lib.load().rmsf_internal_seq_chain_layout
    fn.restype = None
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    out = (ctypes.c_int64 * 5)()
    fn(out)
    return tuple(int(v) for v in out)


g, B, P, R, G = chain_layout()
# 1-5 blocks, whole and ragged: chain_block's two loops, wave_seq_sum's
# two-block loop and its tail, pc_seq_sum's prefetch of blocks past the end
COUNTS = sorted({1, g - 1, g, g + 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 3 * B, 3 * B + 1, 4 * B, 4 * B + 1})
MANY = [B - 1, B, B + 1, 2 * B, 2 * B + 1, 4 * B + 1]  # for the many-frame launch forms
GRID = [G - 1, G, G + 1, G + B, G + B + 1]  # k_ref_seq's last size; k_ref_com_pairs on G/B and G/B + 1 blocks
NF_FEW = 5
IP_SPLIT = P // 10  # the largest two-wave InnerProduct launch


def _forms(c):
    """Frames per launch of c chains each: the last two-wave launch, the first
    and last one-wave launches with reserved LDS, the first unreserved one."""
    return [P // c, P // c + 1, R // c, R // c + 1]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(got, want, what):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _seq(terms, axis):
    """The sequential sum over ``axis``: terms[0] + terms[1] + ... in order."""
    return np.take(np.cumsum(terms, axis=axis), -1, axis=axis)


def _blocked(terms, axis):
    """The same terms summed block by block: each block of B from its first
    term, then the blocks' sums in order -- what a chain restarted per block
    would give."""
    t = np.moveaxis(terms, axis, 0)
    parts = np.stack([_seq(t[a:a + B], 0) for a in range(0, len(t), B)])
    return _seq(parts, 0)


def _order_share(terms, axis, want, what):
    """Assert that the inputs can tell the sequential order from a blocked
    one (more than two blocks only); returns the share of chains that do."""
    if terms.shape[axis] < 2 * B + 1:
        return None
    differ = _bits(_blocked(terms, axis)) != _bits(want)
    print(f"\n{what}: block-by-block sum differs in {int(differ.sum())} of {differ.size} chains")
    assert 2 * int(differ.sum()) >= differ.size, what
    return differ.mean()


def _rows(n, gathered):
    """The selection: the first n atoms, or every 3rd atom of 3 n + 1."""
    return np.arange(1, 3 * n + 1, 3)[:n] if gathered else np.arange(n)


def _masses(n):
    return np.random.default_rng(93).uniform(1.0, 16.0, n)


class _Env:
    def __init__(self, n_atoms, nf, seed):
        from rmsf_amd.engine import Engine
        from rmsf_amd.synth import motion_table
        self.eng = Engine()
        self.host = SY.frames(seed, n_atoms, 0, nf, motion_table(seed + 1, nf))
        self.host.setflags(write=False)
        self.dev = torch.tensor(self.host, device="cuda")
        self.fs = 3 * n_atoms

    def ptr(self, f0=0):
        return self.dev.data_ptr() + 4 * self.fs * f0

    def sel(self, n, gathered):
        return self.eng.sel_tensor(_rows(n, gathered)) if gathered else None


@pytest.fixture(scope="module")
def env():
    """One trajectory for every chain test: R // 3 + 1 frames (the first
    unreserved COM launch) of 3 (4 B + 1) + 1 atoms (the largest gather)."""
    return _Env(3 * max(COUNTS) + 1, R // 3 + 1, 91)


@pytest.fixture(scope="module")
def ref_env():
    """Three frames wide enough for the gathered G + B + 1 atoms."""
    return _Env(3 * max(GRID) + 1, 3, 95)


def _com_want(env, n, gathered, m, nf):
    x = env.host[:nf, _rows(n, gathered)].astype(np.float64)
    terms = x if m is None else x * m[None, :, None]  # f64(x) * m_a; m_a = 1.0 is exact
    mt = float(n) if m is None else float(m.sum())
    return terms, _seq(terms, 1), mt


def _run_com(env, n, gathered, m, mt, f0, nf, xf):
    md = None if m is None else torch.tensor(m, device="cuda")
    env.eng.frame_com_seq(env.ptr(f0), env.fs, nf, n, env.sel(n, gathered), md, mt, xf)


def _ip_want(env, n, gathered, com, ref_c, nf):
    """The ten InnerProduct chains' terms per frame, [nf, n, 10]: A[j] at j,
    G1 at 9, with k_seq_ip's roundings."""
    x1 = env.host[:nf, _rows(n, gathered)].astype(np.float64) - com[:, None, :]
    terms = np.empty((nf, n, 10))
    terms[:, :, :9] = (x1[:, :, :, None] * ref_c[None, :, None, :]).reshape(nf, n, 9)
    terms[:, :, 9] = (x1[:, :, 0] * x1[:, :, 0] + x1[:, :, 1] * x1[:, :, 1]) + x1[:, :, 2] * x1[:, :, 2]
    return x1, terms, _seq(terms, 1)


def _host_reference(env, n, gathered, m):
    """The centred reference of frame 0 and its record, from the oracle and
    sequential sums alone (no kernel involved)."""
    from rmsf_amd._lib import RMSF_REFINFO_DOUBLES
    com0, ref_c = O.centred_reference(env.host[0][_rows(n, gathered)], m)
    info = np.zeros(RMSF_REFINFO_DOUBLES)
    info[0:3] = com0
    info[3:6] = _seq(ref_c, 0)
    info[6] = _seq((ref_c[:, 0] * ref_c[:, 0] + ref_c[:, 1] * ref_c[:, 1]) + ref_c[:, 2] * ref_c[:, 2], 0)
    info[7] = float(n) if m is None else float(m.sum())
    info[8] = float(n)
    return ref_c, info


def _check_qcp(env, n, nf, ref_c, info_d, x1, xf, frames):
    """superpose_seq_qcp on the records: rotation and rmsd of the oracle's
    CalcRMSDRotationalMatrix on the same centred frame and reference."""
    coms = xf[:, 9:12].cpu().numpy()
    env.eng.superpose_seq_qcp(nf, n, info_d, xf)
    torch.cuda.synchronize()
    rec = xf.cpu().numpy()
    _same(rec[:, 9:12], coms, "the QCP leaves the COMs")
    assert not rec[:, 13:16].any()
    for f in frames:
        rot = np.zeros(9)
        rmsd = O.CalcRMSDRotationalMatrix(ref_c, x1[f], n, rot, None)
        _same(rec[f, :9], rot, f"rotation, frame {f}")
        _same(rec[f, 12], rmsd, f"rmsd, frame {f}")


@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("n", COUNTS)
def test_frame_com_chains(env, n, gathered):
    """frame_com_seq's three chains per frame, two-wave form (pc_seq_sum),
    one to five blocks: record [9..11] == (sequential sum of f64(x) m_a) /
    mass_total, with and without masses."""
    from rmsf_amd._lib import RMSF_XFORM_DOUBLES
    for m in (None, _masses(n)):
        terms, sums, mt = _com_want(env, n, gathered, m, NF_FEW)
        if m is not None:
            _order_share(terms, 1, sums, f"COM, n = {n}")
        xf = env.eng.zeros(NF_FEW, RMSF_XFORM_DOUBLES)
        _run_com(env, n, gathered, m, mt, 0, NF_FEW, xf)
        torch.cuda.synchronize()
        rec = xf.cpu().numpy()
        _same(rec[:, 9:12], sums / mt, f"COM, masses {m is not None}")
        assert not rec[:, :9].any() and not rec[:, 12:].any()  # nothing else is written


@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("n", COUNTS)
def test_inner_product_chains(env, n, gathered):
    """inner_product_seq's ten chains per frame, two-wave form, one to five
    blocks, on records holding the frames' COMs: record [j], j < 9, ==
    sequential sum of (f64(x[a, j // 3]) - com[j // 3]) * ref[a, j % 3];
    record [13] == sequential sum of (x1 x1 + y1 y1) + z1 z1.  Then the QCP
    on those records against the oracle's."""
    from rmsf_amd._lib import RMSF_XFORM_DOUBLES
    nf = NF_FEW
    m = _masses(n)
    _, sums, mt = _com_want(env, n, gathered, m, nf)
    com = sums / mt
    ref_c, info = _host_reference(env, n, gathered, m)
    ref_d, info_d = torch.tensor(ref_c, device="cuda"), torch.tensor(info, device="cuda")
    x1, terms, want = _ip_want(env, n, gathered, com, ref_c, nf)
    _order_share(terms, 1, want, f"InnerProduct, n = {n}")
    xf = env.eng.zeros(nf, RMSF_XFORM_DOUBLES)
    _run_com(env, n, gathered, m, mt, 0, nf, xf)
    env.eng.inner_product_seq(env.ptr(), env.fs, nf, n, env.sel(n, gathered), ref_d, xf)
    torch.cuda.synchronize()
    rec = xf.cpu().numpy()
    _same(rec[:, 9:12], com, "COM")
    _same(rec[:, :9], want[:, :9], "A")
    _same(rec[:, 13], want[:, 9], "G1")
    assert not rec[:, 12].any() and not rec[:, 14:].any()
    _check_qcp(env, n, nf, ref_c, info_d, x1, xf, range(nf))


def _in_launches(run, nf, step):
    for f0 in range(0, nf, step):
        run(f0, min(step, nf - f0))


@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("n", MANY)
def test_frame_com_launch_forms(env, n, gathered):
    """The COM chains in every launch form, on both sides of one and two
    blocks and at five: P // 3 frames a launch (two-wave), P // 3 + 1 and
    R // 3 (one wave, reserved LDS), R // 3 + 1 (one wave, unreserved) --
    all the sequential sum's bits, and the largest launch's records equal
    those of the same frames run in two-wave launches."""
    from rmsf_amd._lib import RMSF_XFORM_DOUBLES
    forms = _forms(3)
    top = max(forms)
    for m in (None, _masses(n)):
        terms, sums, mt = _com_want(env, n, gathered, m, top)
        want = sums / mt
        if m is not None:
            _order_share(terms, 1, sums, f"COM, {top} frames, n = {n}")
        recs = {}
        for nf in forms + [0]:  # 0: the largest again, in launches of at most P // 10 frames
            xf = env.eng.zeros(top, RMSF_XFORM_DOUBLES)
            if nf:
                _run_com(env, n, gathered, m, mt, 0, nf, xf)
            else:
                _in_launches(lambda f0, k: _run_com(env, n, gathered, m, mt, f0, k, xf[f0:f0 + k]), top, IP_SPLIT)
            torch.cuda.synchronize()
            recs[nf] = xf.cpu().numpy()
            k = nf or top
            _same(recs[nf][:k, 9:12], want[:k], f"COM, {nf} frames a launch, masses {m is not None}")
            assert not recs[nf][k:].any()
        _same(recs[top], recs[0], "one unreserved launch vs two-wave launches")


@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("n", MANY)
def test_inner_product_launch_forms(env, n, gathered):
    """The InnerProduct chains in every launch form: P // 10 frames a launch
    (two-wave), P // 10 + 1 and R // 10 (one wave, reserved LDS), R // 10 + 1
    (one wave, unreserved -- the form of a 100k-atom, 100-frame run).  The
    one-wave forms run wave_seq_sum, whose two-block loop no other shape
    enters.  Raw sums against the sequential sum; the largest launch's
    records against the same frames in two-wave launches; its QCP against the
    oracle's on the first, a middle and the last frame."""
    from rmsf_amd._lib import RMSF_XFORM_DOUBLES
    forms = _forms(10)
    top = max(forms)
    m = _masses(n)
    _, sums, mt = _com_want(env, n, gathered, m, top)
    com = sums / mt
    ref_c, info = _host_reference(env, n, gathered, m)
    ref_d, info_d = torch.tensor(ref_c, device="cuda"), torch.tensor(info, device="cuda")
    x1, terms, want = _ip_want(env, n, gathered, com, ref_c, top)
    _order_share(terms, 1, want, f"InnerProduct, {top} frames, n = {n}")
    sel = env.sel(n, gathered)
    recs = {}
    for nf in forms + [0]:
        xf = env.eng.zeros(top, RMSF_XFORM_DOUBLES)
        xf[:, 9:12] = torch.tensor(com, device="cuda")  # the COMs are test_frame_com_launch_forms' matter
        if nf:
            env.eng.inner_product_seq(env.ptr(), env.fs, nf, n, sel, ref_d, xf)
        else:
            _in_launches(lambda f0, k: env.eng.inner_product_seq(env.ptr(f0), env.fs, k, n, sel, ref_d, xf[f0:f0 + k]),
                         top, IP_SPLIT)
        torch.cuda.synchronize()
        recs[nf] = xf.cpu().numpy()
        k = nf or top
        _same(recs[nf][:k, :9], want[:k, :9], f"A, {nf} frames a launch")
        _same(recs[nf][:k, 13], want[:k, 9], f"G1, {nf} frames a launch")
        assert not recs[nf][k:, :9].any() and not recs[nf][k:, 12:].any()
    _same(recs[top], recs[0], "one unreserved launch vs two-wave launches")
    _check_qcp(env, n, top, ref_c, info_d, x1, xf, (0, top // 2, top - 1))


def _check_reference(n, m, pos, ref, info, what):
    """The record of reference_setup_seq over the f64 or f32 positions
    ``pos``: COM and centred reference as the oracle's, the sums of the
    centred reference and G2 as sequential sums."""
    mt = float(n) if m is None else float(m.sum())
    com, rc = O.centred_reference(pos, m)
    com_terms = pos.astype(np.float64) * (1.0 if m is None else m[:, None])
    _same(com, _seq(com_terms, 0) / mt, f"{what}: the oracle's COM is the sequential one")
    g2_terms = (rc[:, 0] * rc[:, 0] + rc[:, 1] * rc[:, 1]) + rc[:, 2] * rc[:, 2]
    want_r, want_g2 = _seq(rc, 0), _seq(g2_terms, 0)
    # the COM chains of an unweighted f32 frame sum exactly in any order
    chains = [rc, g2_terms[:, None]] + ([] if m is None and pos.dtype == np.float32 else [com_terms])
    chains = np.concatenate(chains, axis=1)
    _order_share(chains, 0, _seq(chains, 0), f"{what}, n = {n}")
    info = info.cpu().numpy()
    _same(info[0:3], com, f"{what}: ref_com")
    _same(ref.cpu().numpy(), rc, f"{what}: centred reference")
    _same(info[3:6], want_r, f"{what}: sum r")
    _same(info[6], want_g2, f"{what}: G2")
    assert info[7] == mt and info[8] == n and not info[9:16].any()


@pytest.mark.parametrize("source", ["frame", "frame_gathered", "total"])
@pytest.mark.parametrize("n", COUNTS + GRID)
def test_reference_record(ref_env, n, source):
    """reference_setup_seq's record, with and without masses: from a frame
    (contiguous and gathered) and from sweep-1 sums (``total=``).  One to
    five blocks put k_ref_seq's one-wave chains into wave_seq_sum's two-block
    loop; G - 1 is k_ref_seq's last size, and from G the grid-wide fill and
    centring run with k_ref_com_pairs' two-wave COM chains on G / B whole
    blocks, then with a ragged block, then on G / B + 1 and a ragged one."""
    env = ref_env
    gathered = source == "frame_gathered"
    rows = _rows(n, gathered)
    for m in (None, _masses(n)):
        md = None if m is None else torch.tensor(m, device="cuda")
        mt = float(n) if m is None else float(m.sum())
        if source == "total":
            nf = env.host.shape[0]
            total = env.host[:, :n].astype(np.float64).sum(axis=0)
            avg, ref, info = env.eng.reference_setup_seq(n, mt, total=torch.tensor(total.reshape(-1), device="cuda"),
                                                         n_frames=float(nf), masses=md)
            torch.cuda.synchronize()
            pos = total / float(nf)  # RMSF.py:111
            _same(avg.cpu().numpy().reshape(-1, 3), pos, "average")
        else:
            _, ref, info = env.eng.reference_setup_seq(n, mt, frame_ptr=env.ptr(), sel=env.sel(n, gathered), masses=md)
            torch.cuda.synchronize()
            pos = env.host[0][rows]
        _check_reference(n, m, pos, ref, info, f"{source}, masses {m is not None}")
