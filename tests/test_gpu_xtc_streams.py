"""The GPU XTC decoder on hand-built streams with known integers: GPU tier.

scan_wave and what lies under it (the LDS ring and its stages, the
lane-parallel scan of clean groups with its three stop reasons, the carry of
a partly filled batch, the writelane records of the sequential step, ensure()'s
look-ahead, the last partial flush) exist only on the device.  The streams of
tests/xtc_streams.py are built to reach each of them (check_reach, asserted in
tests/test_xtc_streams.py), and the reference is the integers that went into a
stream -- not another decoder.  Both kernels (rmsf_xtc_decode_records and
rmsf_xtc_decode_records_sel) decode every valid stream into a canary-filled
buffer with padding and a guard row; every broken stream leaves NaN in exactly
the frame's values; the host twin's statuses are the device's.
"""
import numpy as np
import pytest

import xtc_streams as Z
from test_gpu_xtc_select import _d2h, _sel_device_decode
from test_xtc_select import CANARY, _row_map
from test_xtc_streams import (BROKEN, K_CORRUPT, VALID, adjacent_pairs, assert_bits_equal, check_selected,
                              check_selected_broken, permuted_selection, sel_host, whole_host)

pytestmark = pytest.mark.gpu


def launch(words, off, ln, n_atoms, pad=0):
    """rmsf_xtc_decode_records into a canary-filled [n + 1 guard row, 3 n_atoms + pad] buffer."""
    import torch

    from rmsf_amd._lib import call
    dev = torch.device("cuda")
    n, stride = len(off), 3 * n_atoms + pad
    d_words = torch.as_tensor(words.view(np.int32)).to(dev)
    d_off, d_ln = torch.as_tensor(off).to(dev), torch.as_tensor(ln).to(dev)
    buf = torch.full((n + 1, stride), float(CANARY), dtype=torch.float32, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    call("rmsf_xtc_decode_records", d_words.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), n, n_atoms,
         buf.data_ptr(), stride, st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), st.cpu().numpy()


def pack(frames, gap=()):
    """The records one after another (gap[k] unused words in front of record
    k): words, rec_off, rec_len."""
    parts, off, ln, at = [], [], [], 0
    for k, f in enumerate(frames):
        g = gap[k] if k < len(gap) else 0
        parts.append(np.full(g, 0xDEADBEEF, dtype=np.uint32))
        w = np.frombuffer(f.record, dtype=np.uint32)
        parts.append(w)
        off.append(at + g)
        ln.append(len(w))
        at += g + len(w)
    return np.concatenate(parts), np.array(off, dtype=np.int64), np.array(ln, dtype=np.int64)


def whole_device(frame, pad=3):
    buf, st = launch(*Z.words_of(frame), frame.declared, pad)
    return buf, int(st[0])


def sel_device(frame, sel, pad=0):
    words, off, ln = Z.words_of(frame)
    buf, st = _sel_device_decode(words, off, ln, frame.declared, np.ascontiguousarray(sel, dtype=np.int32), pad)
    return buf, int(st[0])


def check_whole(buf, st, want, pad, row=0, rows=1):
    n3 = want.size
    assert st == 0
    assert_bits_equal(buf[row, :n3].reshape(-1, 3), want)
    assert (buf[row, n3:] == CANARY).all() and (buf[rows] == CANARY).all() and buf.shape == (rows + 1, n3 + pad)


# -- valid streams ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", VALID)
def test_whole_frame_kernel_gives_the_built_integers(name):
    f = Z.stream(name)
    buf, st = whole_device(f, pad=3)
    assert st == whole_host(f)[1]
    check_whole(buf, st, Z.expected(name), 3)


@pytest.mark.parametrize("name", VALID)
def test_selection_kernel_gives_the_built_integers(name):
    """A third of the atoms in random order: the selection kernel on every
    stream, those past the ring (more than 4,096 words) included."""
    f, want = Z.stream(name), Z.expected(name)
    sel = permuted_selection(f.n_atoms, 1 / 3, 13)
    buf, st = sel_device(f, sel, pad=3)
    ref, st_ref = sel_host(f, sel, pad=3)
    assert st == st_ref
    check_selected(buf, st, want, sel, 3)
    assert_bits_equal(buf, ref)  # rows, padding and guard row alike


@pytest.mark.parametrize("fraction", [0.02, 0.5, 1.0])
@pytest.mark.parametrize("name", ["mixed", "index_walk_w72"])
def test_random_permuted_selection(name, fraction):
    f, want = Z.stream(name), Z.expected(name)
    sel = permuted_selection(f.n_atoms, fraction, 11)
    buf, st = sel_device(f, sel, pad=5)
    check_selected(buf, st, want, sel, 5)


def _many_selections(frame, want, sels, pad):
    """One tiny launch per selection; the record is uploaded once."""
    import torch

    from rmsf_amd._lib import call
    dev = torch.device("cuda")
    words, off, ln = Z.words_of(frame)
    d_words = torch.as_tensor(words.view(np.int32)).to(dev)
    d_off, d_ln = torch.as_tensor(off).to(dev), torch.as_tensor(ln).to(dev)
    s = torch.cuda.current_stream().cuda_stream
    for sel in sels:
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        stride = 3 * len(sel) + pad
        d_map = torch.as_tensor(_row_map(sel, frame.n_atoms)).to(dev)
        buf = torch.full((2, stride), float(CANARY), dtype=torch.float32, device=dev)
        st = torch.full((1,), -1, dtype=torch.int32, device=dev)
        call("rmsf_xtc_decode_records_sel", d_words.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), 1, frame.n_atoms,
             d_map.data_ptr(), len(sel), buf.data_ptr(), stride, st.data_ptr(), s)
        torch.cuda.synchronize()
        check_selected(buf.cpu().numpy(), int(st.cpu()[0]), want, sel, pad)


def test_every_single_atom_of_every_run_length():
    f, want = Z.stream("runs_0_to_10"), Z.expected("runs_0_to_10")
    _many_selections(f, want, [[a] for a in range(f.n_atoms)], pad=2)


def test_every_adjacent_pair_in_both_orders():
    f, want = Z.stream("runs_0_to_10"), Z.expected("runs_0_to_10")
    _many_selections(f, want, adjacent_pairs(f.n_atoms), pad=1)


# -- broken streams ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BROKEN)
def test_broken_stream_whole_frame_kernel(name):
    """All 3 n_atoms values are NaN, the rows that earlier batches had written
    included (the long forms); padding and guard row keep the canary."""
    f = Z.stream(name)
    n3 = 3 * f.declared
    buf, st = whole_device(f, pad=4)
    assert st == K_CORRUPT == whole_host(f)[1]
    assert np.isnan(buf[0, :n3]).all()
    assert (buf[0, n3:] == CANARY).all() and (buf[1] == CANARY).all()


@pytest.mark.parametrize("name", BROKEN)
def test_broken_stream_selection_kernel(name):
    f = Z.stream(name)
    sel = permuted_selection(f.declared, 0.3, 7)
    buf, st = sel_device(f, sel, pad=4)
    ref, st_ref = sel_host(f, sel, pad=4)
    assert st == st_ref
    check_selected_broken(buf, st, len(sel))
    np.testing.assert_array_equal(buf, ref)  # NaN positions compare equal


# -- several records in one launch ---------------------------------------------------------------------

def test_broken_record_disturbs_neither_neighbour():
    """Frames are blocks of one launch: a long valid record, the same groups
    broken behind word 4,608, a short valid one -- equal atom counts,
    different headers and lengths."""
    frames = Z.mixed_launch_frames()
    ok, bad, short = frames
    n, n3 = ok.n_atoms, 3 * ok.n_atoms
    words, off, ln = pack(frames, gap=(0, 1, 0))
    buf, st = launch(words, off, ln, n, pad=2)
    assert st.tolist() == [0, K_CORRUPT, 0]
    check_whole(buf, 0, Z.expected_angstrom(ok.ints, ok.precision), 2, row=0, rows=3)
    check_whole(buf, 0, Z.expected_angstrom(short.ints, short.precision), 2, row=2, rows=3)
    assert np.isnan(buf[1, :n3]).all() and (buf[1, n3:] == CANARY).all()
    sel = permuted_selection(n, 0.1, 3)
    got, st = _sel_device_decode(words, off, ln, n, sel, pad=2)
    assert st.tolist() == [0, K_CORRUPT, 0]
    k3 = 3 * len(sel)
    assert_bits_equal(got[0, :k3].reshape(-1, 3), Z.expected_angstrom(ok.ints, ok.precision)[sel])
    assert_bits_equal(got[2, :k3].reshape(-1, 3), Z.expected_angstrom(short.ints, short.precision)[sel])
    assert np.isnan(got[1, :k3]).all() and (got[:3, k3:] == CANARY).all() and (got[3] == CANARY).all()


def test_two_records_around_the_stage_size():
    """Streams of 511 and 513 words (one word per atom) in one buffer, the
    second record at an odd word offset.  The atom count belongs to the
    launch, so each record is launched from the shared buffer on its own."""
    a, b = Z.stream("word_per_atom_511"), Z.stream("word_per_atom_513")
    words, off, ln = pack([a, b], gap=(0, 1))
    assert off[1] % 2 == 1 and a.n_words == 511 and b.n_words == 513
    for k, name in enumerate(("word_per_atom_511", "word_per_atom_513")):
        f = Z.stream(name)
        buf, st = launch(words, off[k:k + 1], ln[k:k + 1], f.n_atoms, pad=1)
        check_whole(buf, int(st[0]), Z.expected(name), 1)
        sel = permuted_selection(f.n_atoms, 0.25, 5)
        got, st = _sel_device_decode(words, off[k:k + 1], ln[k:k + 1], f.n_atoms, sel, pad=1)
        check_selected(got, int(st[0]), Z.expected(name), sel, 1)


# -- the pinned-slot decoder ---------------------------------------------------------------------------

def test_pinned_slot_decoder_gives_the_built_integers(tmp_path):
    """A file of five frames of one atom count under three kinds of header
    (packed <= 52 bits, packed 72 bits, per axis): decode and decode_list,
    whole frames and a permuted selection."""
    import torch

    from rmsf_amd.sources import XtcDecoder
    from rmsf_amd.xtc import XTCFile
    kinds = Z.shared_natoms_frames()
    frames = [kinds[k] for k in (0, 1, 2, 1, 0)]
    want = np.stack([Z.expected_angstrom(f.ints, f.precision) for f in frames])
    n = kinds[0].n_atoms
    p = tmp_path / "kinds.xtc"
    p.write_bytes(b"".join(f.record for f in frames))
    s = torch.cuda.current_stream().cuda_stream
    lst = np.array([4, 1, 1, 2, 0], dtype=np.int64)
    with XTCFile(str(p)) as x:
        assert (x.n_atoms, x.n_frames) == (n, 5)
        for sel in (None, permuted_selection(n, 0.2, 9)):
            rows = n if sel is None else len(sel)
            ref = want if sel is None else want[:, sel]
            dec = XtcDecoder(x, batch_frames=3, n_slots=2, n_threads=2, sel=sel)
            for first, count, step in ((0, 3, 1), (3, 2, 1), (0, 3, 2)):
                slot, ptr = dec.decode(first, count, step, s)
                assert_bits_equal(_d2h(ptr, (count, rows, 3), s), ref[first:first + count * step:step])
                dec.release(slot, s)
            for part in (lst[:3], lst[3:]):
                slot, ptr = dec.decode_list(part, s)
                assert_bits_equal(_d2h(ptr, (len(part), rows, 3), s), ref[part])
                dec.release(slot, s)
            dec.synchronize()
            dec.close()
