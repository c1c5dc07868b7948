"""The XTC decoders on hand-built streams with known integers: CPU tier.

Every other XTC test decodes what the project's own writer wrote, and its
reference is another decoder.  Here the streams come from tests/xtc_streams.py,
a plain-Python encoder of explicit groups, and the reference is the integers
that went in (expected_angstrom): small triples of every width 9..72 inside
runs (53..72 bits: the byte division in pass 2), runs of 9 and 10, large
triples from 1 bit to 72 packed and 96 per axis, chosen lengths of flag-free
stretches, stream lengths around the device's 512-word stages and 4,096-word
ring, the index resting at 8, and streams broken in one known place.

This file holds the device decoder's code as compiled for the host
(rmsf_xtc_decode_records_host, rmsf_xtc_decode_records_sel_host), the host
codec (XTCFile.read) and the independent Python decoder (oracle.xtc_py) to
those integers, bit for bit, and checks that each zoo stream reaches what it
is for (xtc_streams.check_reach).  tests/test_gpu_xtc_streams.py holds the
device kernels to the same.
"""
import numpy as np
import pytest

import xtc_streams as Z
from test_xtc_gpu import _host_decode
from test_xtc_select import CANARY, _sel_host_decode

K_CORRUPT = 5  # xtc_gpu.hip's kCorrupt: what every broken stream of the zoo is
VALID, BROKEN = sorted(Z.VALID), sorted(Z.BROKEN)
# oracle.xtc_py reads bit by bit in Python: the streams above 10,000 words are left to the other two decoders
ORACLE_SKIPPED = {"mixed"}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits_equal(got, want):
    np.testing.assert_array_equal(bits(got), bits(want))


def whole_host(frame):
    words, off, ln = Z.words_of(frame)
    out, st = _host_decode(words, off, ln, frame.declared)
    return out[0], int(st[0])


def sel_host(frame, sel, pad=0):
    words, off, ln = Z.words_of(frame)
    buf, st = _sel_host_decode(words, off, ln, frame.declared, np.ascontiguousarray(sel, dtype=np.int32), pad)
    return buf, int(st[0])


def check_selected(buf, st, want, sel, pad):
    """Status 0, the rows are want[sel] bit for bit, everything else still the canary."""
    assert st == 0
    assert_bits_equal(buf[0, :3 * len(sel)].reshape(len(sel), 3), want[sel])
    assert (buf[0, 3 * len(sel):] == CANARY).all() and (buf[1] == CANARY).all()
    assert buf.shape == (2, 3 * len(sel) + pad)


def check_selected_broken(buf, st, n_sel):
    """Status kCorrupt, NaN in exactly the 3 n_sel values, the canary elsewhere."""
    assert st == K_CORRUPT
    assert np.isnan(buf[0, :3 * n_sel]).all()
    assert (buf[0, 3 * n_sel:] == CANARY).all() and (buf[1] == CANARY).all()


def permuted_selection(n_atoms, fraction, seed):
    rng = np.random.default_rng(seed)
    return rng.permutation(n_atoms)[:max(1, int(round(fraction * n_atoms)))].astype(np.int32)


def adjacent_pairs(n_atoms):
    return [[a, a + 1] for a in range(n_atoms - 1)] + [[a + 1, a] for a in range(n_atoms - 1)]


@pytest.fixture(scope="module")
def stream_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("xtc_streams")


def _file(stream_dir, name):
    p = stream_dir / f"{name}.xtc"
    if not p.exists():
        p.write_bytes(Z.stream(name).record)
    return str(p)


# -- the builder ------------------------------------------------------------------------

def test_builder_refusals():
    lo, hi = Z.HEADERS["w38"]
    v = Z.Values(1)
    with pytest.raises(ValueError, match="fewer than 10"):
        Z.build_frame(lo, hi, 20, 1000.0, [(2, 0)] * 3, v)
    with pytest.raises(ValueError, match="index 8"):
        Z.build_frame(lo, hi, 9, 1000.0, [(0, -1), (1, 0)] + [(0, 0)] * 10, v)
    with pytest.raises(ValueError, match="int32"):  # a small offset on top of maxint = 2^31 - 2 wraps in C
        Z.build_frame((Z.I32_MIN, 0, 0), (Z.I32_MAX - 1, 9, 9), 72, 1000.0, [(10, 0)] * 40, v)
    with pytest.raises(ValueError, match="run code"):  # 3*10 + 1 + 1 = 32 does not fit 5 bits
        Z.build_frame(lo, hi, 20, 1000.0, [(10, 1)] * 4, v)
    with pytest.raises(ValueError, match="left the table"):
        Z.build_frame(lo, hi, 72, 1000.0, [(2, 0)] * 6 + [(2, 1), (2, 0)], v)


def test_builder_bit_layout():
    """One group spelt out by hand: the packed triple's byte order, the flag
    code, the water swap, the header fields."""
    class Fixed:
        def __init__(self, seq):
            self.seq = list(seq)

        def triple(self, sizes):
            return self.seq.pop(0)

    # sizeint (5, 6, 7): 210 -> 8 bits; index 12: magic 16, half 8, 12-bit small triples
    groups = [(2, 0)] + [(0, 0)] * 8
    seq = [[4, 5, 6], [1, 2, 3], [15, 0, 9]] + [[0, 0, 0]] * 8
    f = Z.build_frame((10, 20, 30), (14, 25, 36), 12, 1000.0, groups, Fixed(seq))
    assert f.large_bits == 8 and f.n_atoms == 11
    big = (4 * 6 + 5) * 7 + 6                  # 209: one byte
    t0 = (1 * 16 + 2) * 16 + 3                 # 0x123: low byte 0x23 first, then the top 4 bits 0x1
    t1 = (15 * 16 + 0) * 16 + 9                # 0xf09: 0x09, then 0xf
    want = f"{big:08b}" + "1" + f"{3 * 2 + 0 + 1:05b}" + f"{0x23:08b}{0x1:04b}" + f"{0x09:08b}{0xf:04b}"
    want += ("00000000" + "1" + f"{1:05b}") + ("00000000" + "0") * 7  # run back to 0 (flagged), then clean
    stream = f.record[92:92 + f.nbytes]
    got = "".join(f"{b:08b}" for b in stream)
    assert got[:len(want)] == want and set(got[len(want):]) <= {"0"} and f.stream_bits == len(want)
    assert f.ints[:3].tolist() == [[14 + 1 - 8, 25 + 2 - 8, 36 + 3 - 8], [14, 25, 36],
                                   [14 + 1 - 8 + 15 - 8, 25 + 2 - 8 - 8, 36 + 3 - 8 + 9 - 8]]
    assert f.layout[0] == Z.Group(0, 0, 12, 2, True, 8 + 6 + 24) and f.layout[1].atom == 3
    assert int.from_bytes(f.record[4:8], "big") == 11 == int.from_bytes(f.record[52:56], "big")
    assert int.from_bytes(f.record[84:88], "big") == 12 and int.from_bytes(f.record[88:92], "big") == f.nbytes


def test_expected_angstrom_rounding():
    i = np.array([[0, 1, -1], [12345678, -2**31, 2**31 - 1]], dtype=np.int64)
    for prec in (1000.0, 1234.5):
        inv = np.float32(1.0 / float(np.float32(prec)))
        want = [[np.float32(np.float32(np.float32(int(x)) * inv) * np.float32(10)) for x in row] for row in i]
        assert_bits_equal(Z.expected_angstrom(i, prec), np.array(want, dtype=np.float32))


@pytest.mark.parametrize("name", VALID + BROKEN)
def test_stream_reaches_what_it_is_for(name):
    Z.check_reach(name)


def test_zoo_is_complete():
    assert {f"index_walk_{h}" for h in Z.WALK_HEADERS} <= set(VALID)
    assert {f"word_per_atom_{n}" for n in (511, 512, 513, 4095, 4096, 4097, 4607, 4608, 4609, 8193)} <= set(VALID)
    assert len([n for n in VALID if n.startswith("bitsize_edges")]) == 12
    assert len([n for n in VALID if n.startswith("clean_")]) == 8
    assert Z.BROKEN_CLASSES == sorted(["nbytes-1_clean", "nbytes-8_clean", "nbytes-1_flagged", "run_past_natoms",
                                       "ends_before_natoms", "run_at_8", "index_to_7", "index_to_73"])
    assert set(BROKEN) == {f"{c}_{s}" for c in Z.BROKEN_CLASSES for s in ("short", "long")}
    assert {n for n in VALID if Z.stream(n).n_words > 10000} == ORACLE_SKIPPED
    for s in ("short", "long"):  # the exact-length twin: the same bytes but for the count and the cut
        a, b = Z.stream(f"exact_flagged_{s}"), Z.stream(f"nbytes-1_flagged_{s}")
        assert a.nbytes == b.nbytes + 1 and a.record[92:92 + b.nbytes] == b.record[92:92 + b.nbytes]
    frames = Z.shared_natoms_frames()
    assert len({f.n_atoms for f in frames}) == 1 and [f.large_bits for f in frames] == [38, 72, 62]
    ok, bad, short = Z.mixed_launch_frames()
    assert ok.n_atoms == bad.n_atoms == short.n_atoms and bad.nbytes == (bad.stream_bits + 7) // 8 - 1
    assert min(ok.n_words, bad.n_words) > Z.LONG_WORDS and short.n_words < ok.n_words // 2


# -- valid streams: three decoders, the built integers ----------------------------------------

@pytest.mark.parametrize("name", VALID)
def test_host_twin_gives_the_built_integers(name):
    got, st = whole_host(Z.stream(name))
    assert st == 0
    assert_bits_equal(got, Z.expected(name))


@pytest.mark.parametrize("name", VALID)
def test_host_codec_gives_the_built_integers(stream_dir, name):
    from rmsf_amd.xtc import XTCFile
    with XTCFile(_file(stream_dir, name)) as f:
        assert (f.n_atoms, f.n_frames) == (Z.stream(name).n_atoms, 1)
        assert_bits_equal(f.read()[0], Z.expected(name))


@pytest.mark.parametrize("name", [n for n in VALID if n not in ORACLE_SKIPPED])
def test_python_decoder_gives_the_built_integers(stream_dir, name):
    from oracle.xtc_py import read_xtc
    got = read_xtc(_file(stream_dir, name))
    assert got.shape[0] == 1
    assert_bits_equal(got[0], Z.expected(name))


# -- broken streams ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", BROKEN)
def test_broken_stream_is_rejected(stream_dir, name):
    from rmsf_amd import RmsfError
    from rmsf_amd.xtc import XTCFile
    f = Z.stream(name)
    got, st = whole_host(f)
    assert st == K_CORRUPT
    sel = permuted_selection(f.declared, 0.3, 7)
    buf, st_sel = sel_host(f, sel, pad=4)
    check_selected_broken(buf, st_sel, len(sel))
    with pytest.raises(RmsfError):
        with XTCFile(_file(stream_dir, name)) as x:
            x.read()


# -- selections ----------------------------------------------------------------------------------

def test_every_single_atom_of_every_run_length():
    """One group of each run length 0..10, each of its 66 atoms selected alone:
    every branch of MapRows::triples at every position."""
    f, want = Z.stream("runs_0_to_10"), Z.expected("runs_0_to_10")
    for a in range(f.n_atoms):
        buf, st = sel_host(f, [a], pad=2)
        check_selected(buf, st, want, np.array([a]), 2)


def test_every_adjacent_pair_in_both_orders():
    f, want = Z.stream("runs_0_to_10"), Z.expected("runs_0_to_10")
    for pair in adjacent_pairs(f.n_atoms):
        buf, st = sel_host(f, pair, pad=1)
        check_selected(buf, st, want, np.array(pair), 1)


@pytest.mark.parametrize("fraction", [0.02, 0.5])
@pytest.mark.parametrize("name", ["mixed", "index_walk_w72"])
def test_random_permuted_selection(name, fraction):
    f, want = Z.stream(name), Z.expected(name)
    sel = permuted_selection(f.n_atoms, fraction, 11)
    assert len(set(sel.tolist())) == len(sel) and (np.diff(sel) < 0).any()
    buf, st = sel_host(f, sel, pad=5)
    check_selected(buf, st, want, sel, 5)


def test_file_of_three_header_kinds(tmp_path):
    """Frames of one atom count under three kinds of header in one file (what
    the GPU tier feeds to the pinned-slot decoder): host codec and host twin."""
    from rmsf_amd.xtc import XTCFile
    from test_xtc_gpu import _records
    frames = Z.shared_natoms_frames()
    want = np.stack([Z.expected_angstrom(f.ints, f.precision) for f in frames])
    p = tmp_path / "kinds.xtc"
    p.write_bytes(b"".join(f.record for f in frames))
    sel = permuted_selection(frames[0].n_atoms, 0.2, 9)
    with XTCFile(str(p)) as x:
        assert (x.n_atoms, x.n_frames) == (frames[0].n_atoms, 3)
        assert_bits_equal(x.read(), want)
        assert_bits_equal(x.read(sel=sel), want[:, sel])
    words, off, ln, n_atoms = _records(str(p))
    got, st = _host_decode(words, off, ln, n_atoms)
    assert (st == 0).all()
    assert_bits_equal(got, want)
    ok, bad, short = Z.mixed_launch_frames()
    assert [whole_host(f)[1] for f in (ok, bad, short)] == [0, K_CORRUPT, 0]
    assert_bits_equal(whole_host(short)[0], Z.expected_angstrom(short.ints, short.precision))
