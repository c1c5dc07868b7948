"""Selection-aware XTC decode (csrc/xtc_gpu.hip, the *_sel entries): CPU tier.

RMSF.py keeps 214 CA atoms of 47,681 (RMSF.py:77,126).  The selected decoder
writes those atoms only, through a map atom -> output row.  Here its code,
run on the host (rmsf_xtc_decode_records_sel_host), must give the bits of the
whole-frame decoder's [:, sel] and of the independent host codec
(XTCFile.read(sel=...)) for every compression path of test_xtc_gpu._cases()
and every shape of selection that takes another way through a group: nothing
selected in it, a run cut after its last selected atom, either atom of the
writer's water swap alone, a permutation.  It must write nothing but the
selected rows (canary), and reject exactly what the whole-frame decoder
rejects.  tests/test_gpu_xtc_select.py holds the device kernel to this twin.
"""
import functools
import struct

import numpy as np
import pytest

from test_xtc import _protein_like
from test_xtc_gpu import _cases, _host_decode, _records

CANARY = np.float32(-12345.5)


def _run_groups(path, frame=0):
    """[(first atom, small triples)] of the groups of one compressed frame: the
    flag walk alone (pass 1), written from the published format with the
    independent Python decoder's helpers.  [] for a raw (<= 9 atoms) frame."""
    from oracle.xtc_py import _Bits, _sizeofint, _sizeofints
    from rmsf_amd.xtc import XTCFile
    with XTCFile(path) as f:
        off, nbytes = f.record(frame)
        natoms = f.n_atoms
    data = open(path, "rb").read()[off:off + nbytes]
    if natoms <= 9:
        return []
    p = 56  # magic natoms step time box[9] lsize
    minint = struct.unpack(">iii", data[p + 4:p + 16])
    maxint = struct.unpack(">iii", data[p + 16:p + 28])
    smallidx, nb = struct.unpack(">ii", data[p + 28:p + 36])
    bs = _Bits(data[p + 36:p + 36 + nb])
    sizeint = [maxint[i] - minint[i] + 1 for i in range(3)]
    if (sizeint[0] | sizeint[1] | sizeint[2]) > 0xFFFFFF:
        large_bits = sum(_sizeofint(s) for s in sizeint)
    else:
        large_bits = _sizeofints(sizeint)
    groups, i, run = [], 0, 0
    while i < natoms:
        bs.pos += large_bits
        is_smaller = 0
        if bs.bits(1):
            run = bs.bits(5)
            is_smaller = run % 3
            run -= is_smaller
            is_smaller -= 1
        groups.append((i, run // 3))
        bs.pos += (run // 3) * smallidx
        i += 1 + run // 3
        smallidx += is_smaller
    assert i == natoms
    return groups


@functools.lru_cache(maxsize=None)
def _case(case, tmp):
    """One XTC per case, written and decoded (whole frames) once per session:
    (path, words, off, ln, n_atoms, whole-frame host decode, groups of frame 0)."""
    from rmsf_amd.xtc import write_xtc
    x, prec = _cases()[case]
    p = f"{tmp}/{case}.xtc"
    write_xtc(p, x, precision=prec)
    words, off, ln, n_atoms = _records(p)
    full, st = _host_decode(words, off, ln, n_atoms)
    assert (st == 0).all()
    full.setflags(write=False)
    return p, words, off, ln, n_atoms, full, _run_groups(p)


@pytest.fixture(scope="session")
def xtc_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("xtc_select"))


def _selections(n_atoms, groups):
    """name -> int32 selection, each where it is defined for the case."""
    s = {
        "every10th": np.arange(0, n_atoms, 10),
        "first": np.array([0]),
        "last": np.array([n_atoms - 1]),
        "reversed": np.arange(n_atoms)[::-1],
        "one": np.array([n_atoms // 2]),
    }
    runs = [(i, ns) for i, ns in groups if ns >= 1]
    if runs:  # the writer swapped atoms i and i+1 of each run
        i, _ = runs[len(runs) // 2]
        s["swap_first"] = np.array([i])
        s["swap_second"] = np.array([i + 1])
        s["swap_both_reversed"] = np.array([i + 1, i])
    long_runs = [i for i, ns in groups if ns >= 2]  # runs of >= 3 atoms
    if len(long_runs) >= 2:  # from the second atom of one run to the second atom of a later one
        s["block"] = np.arange(long_runs[0] + 1, long_runs[-1] + 2)
    else:
        s["block"] = np.arange(n_atoms // 3, 2 * n_atoms // 3)
    if n_atoms <= 9:
        s["raw_subset"] = np.array([7, 2, 3])
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in s.items()}


COMMON = ["every10th", "first", "last", "block", "reversed", "one"]
SWAPS = ["swap_first", "swap_second", "swap_both_reversed"]
RUN_CASES = sorted(set(_cases()) - {"raw9"})  # every compressed case has a run in frame 0 (checked below)


def _defined(case):
    """The selections defined for a case (test_selections_cover_the_group_paths
    checks this against what _selections() finds in the file)."""
    return COMMON + (SWAPS if case in RUN_CASES else []) + (["raw_subset"] if case == "raw9" else [])


CASE_SEL = [(c, n) for c in sorted(_cases()) for n in _defined(c)]


def _row_map(sel, n_atoms):
    m = np.full(n_atoms, -1, dtype=np.int32)
    m[sel] = np.arange(len(sel), dtype=np.int32)
    return m


def _sel_host_decode(words, off, ln, n_atoms, sel, pad=0):
    """(buffer [n + 1 guard frame, 3 n_sel + pad] pre-filled with the canary,
    statuses): frame f's selected rows at buffer[f, :3 n_sel]."""
    from rmsf_amd._lib import call
    n, stride = len(off), 3 * len(sel) + pad
    buf = np.full((n + 1, stride), CANARY, dtype=np.float32)
    st = np.full(n, -1, dtype=np.int32)
    m = _row_map(sel, n_atoms)
    call("rmsf_xtc_decode_records_sel_host", words.ctypes.data, off.ctypes.data, ln.ctypes.data, n, n_atoms,
         m.ctypes.data, len(sel), buf.ctypes.data, stride, st.ctypes.data)
    return buf, st


def _case_sel(case, name, xtc_dir):
    p, words, off, ln, n_atoms, full, groups = _case(case, xtc_dir)
    return p, words, off, ln, n_atoms, full, _selections(n_atoms, groups)[name]


def test_selections_cover_the_group_paths(xtc_dir):
    """The cases give the selections something to cut: runs with a water swap,
    more than 64 groups per frame (full and partial 64-group flushes), a raw
    case, and both atoms of a swapped pair on their own."""
    *_, n_atoms, _, groups = _case("protein", xtc_dir)
    assert len(groups) > 64 and len(groups) % 64 != 0
    sels = _selections(n_atoms, groups)
    a, b = int(sels["swap_first"][0]), int(sels["swap_second"][0])
    assert b == a + 1 and (a, True) in [(i, ns >= 1) for i, ns in groups]
    assert sels["swap_both_reversed"].tolist() == [b, a]
    long_runs = [i for i, ns in groups if ns >= 2]
    blk = sels["block"]  # starts and ends inside runs of three atoms
    assert blk[0] == long_runs[0] + 1 and blk[-1] == long_runs[-1] + 1 and long_runs[-1] > long_runs[0]
    for case in _cases():
        *_, n, _, g = _case(case, xtc_dir)
        assert sorted(_selections(n, g)) == sorted(_defined(case)), case


@pytest.mark.parametrize("case,name", CASE_SEL)
def test_selected_host_twin_matches_whole_frame_decode(xtc_dir, case, name):
    from rmsf_amd.xtc import XTCFile
    p, words, off, ln, n_atoms, full, sel = _case_sel(case, name, xtc_dir)
    buf, st = _sel_host_decode(words, off, ln, n_atoms, sel)
    assert (st == 0).all()
    got = buf[:-1].reshape(len(off), len(sel), 3)
    np.testing.assert_array_equal(got, full[:, sel])
    with XTCFile(p) as f:
        np.testing.assert_array_equal(got, f.read(sel=sel))
    assert (buf[-1] == CANARY).all()


@pytest.mark.parametrize("case,name", [("protein", "every10th"), ("protein", "swap_second"), ("protein", "block"),
                                       ("raw9", "raw_subset"), ("ten", "one"), ("large_range", "every10th"),
                                       ("wide60", "reversed")])
def test_padding_and_guard_row_untouched(xtc_dir, case, name):
    """out_stride > 3 n_sel: nothing is written outside the selected rows."""
    p, words, off, ln, n_atoms, full, sel = _case_sel(case, name, xtc_dir)
    buf, st = _sel_host_decode(words, off, ln, n_atoms, sel, pad=5)
    assert (st == 0).all()
    np.testing.assert_array_equal(buf[:-1, :3 * len(sel)].reshape(len(off), len(sel), 3), full[:, sel])
    assert (buf[:-1, 3 * len(sel):] == CANARY).all() and (buf[-1] == CANARY).all()


def _corrupt500(tmp_path):
    """test_xtc_gpu.test_corrupt_records_are_rejected's file and its three corruptions."""
    from rmsf_amd.xtc import write_xtc
    p = str(tmp_path / "t.xtc")
    write_xtc(p, _protein_like(np.random.default_rng(2), 500, 3))
    words, off, ln, n_atoms = _records(p)
    bad = words.copy()
    bad[off[0]] = 0                                   # frame 0: magic
    bad[off[1] + 1] = bad[off[1] + 1] ^ 0x01000000    # frame 1: atom count
    ln2 = ln.copy()
    ln2[2] = 30                                       # frame 2: truncated record
    return words, bad, off, ln, ln2, n_atoms


def test_corrupt_records_same_status_nan_rows_only(tmp_path):
    _, bad, off, _, ln2, n_atoms = _corrupt500(tmp_path)
    _, st_full = _host_decode(bad, off, ln2, n_atoms)
    sel = np.arange(3, n_atoms, 7, dtype=np.int32)[::-1].copy()
    buf, st = _sel_host_decode(bad, off, ln2, n_atoms, sel, pad=4)
    assert (st_full != 0).all()
    np.testing.assert_array_equal(st, st_full)
    assert np.isnan(buf[:-1, :3 * len(sel)]).all()           # exactly the n_sel rows ...
    assert (buf[:-1, 3 * len(sel):] == CANARY).all() and (buf[-1] == CANARY).all()   # ... and never more


def test_garbage_streams_same_decision_same_atoms(tmp_path):
    """60 random garbage streams: the selected decoder accepts exactly what the
    whole-frame decoder accepts, gives the same selected atoms, never crashes."""
    words, _, off, ln, _, n_atoms = _corrupt500(tmp_path)
    rng = np.random.default_rng(0)
    sel = np.sort(np.random.default_rng(3).choice(n_atoms, 40, replace=False)).astype(np.int32)
    n_ok = 0
    for t in range(60):
        g = words.copy()
        lo = off[0] + 24 + (t % 5) * 40  # corrupt from a few depths into the stream
        g[lo:off[0] + ln[0]] = rng.integers(0, 2**32, off[0] + ln[0] - lo, dtype=np.uint64).astype(np.uint32)
        full, st_full = _host_decode(g, off[:1], ln[:1], n_atoms)
        buf, st = _sel_host_decode(g, off[:1], ln[:1], n_atoms, sel)
        assert st[0] == st_full[0], t
        assert (buf[-1] == CANARY).all()
        if st[0] == 0:
            n_ok += 1
            np.testing.assert_array_equal(buf[0].reshape(-1, 3), full[0][sel])
        else:
            assert np.isnan(buf[0]).all()
    assert 0 < n_ok < 60  # both outcomes exercised


def test_bad_map_is_rejected(xtc_dir):
    from rmsf_amd import RmsfError
    from rmsf_amd._lib import call
    _, words, off, ln, n_atoms, _, _ = _case("ten", xtc_dir)
    out = np.zeros((len(off), 2, 3), dtype=np.float32)
    st = np.zeros(len(off), dtype=np.int32)
    m = np.full(n_atoms, -1, dtype=np.int32)
    m[4] = 2  # a row past n_sel = 2
    with pytest.raises(RmsfError):
        call("rmsf_xtc_decode_records_sel_host", words.ctypes.data, off.ctypes.data, ln.ctypes.data, len(off), n_atoms,
             m.ctypes.data, 2, out.ctypes.data, 6, st.ctypes.data)
    m[4] = 1
    with pytest.raises(RmsfError):  # out_stride < 3 n_sel
        call("rmsf_xtc_decode_records_sel_host", words.ctypes.data, off.ctypes.data, ln.ctypes.data, len(off), n_atoms,
             m.ctypes.data, 2, out.ctypes.data, 5, st.ctypes.data)


def test_source_rejects_duplicates_for_selected_decode(xtc_dir):
    """decode_select=True with an atom listed twice: ValueError, before any
    device work (this runs without a GPU)."""
    from rmsf_amd.sources import XtcSource
    p = _case("ten", xtc_dir)[0]
    with pytest.raises(ValueError, match="twice"):
        XtcSource(p, np.array([1, 4, 4]), decode_select=True)
    with pytest.raises(ValueError):
        XtcSource(p, None, decode_select=True)
    with pytest.raises(ValueError):
        XtcSource(p, np.array([1, 4]), decode="host", decode_select=True)
