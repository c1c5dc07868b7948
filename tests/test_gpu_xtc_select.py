"""Selection-aware XTC decode on the device (GPU tier).

The kernel (rmsf_xtc_decode_records_sel) is held to its host twin, which
tests/test_xtc_select.py holds to the whole-frame decoder and the host codec;
the pinned-slot decoder (XtcDecoder(sel=...)), XtcSource(decode_select=...),
its HBM cache and the context's rmsf_push_xtc are held to the host-decoded
selected frames, bit for bit wherever both legs feed the same batches."""
import numpy as np
import pytest

from test_xtc import _protein_like
from test_xtc_gpu import _host_decode, _records
from test_xtc_select import CANARY, CASE_SEL, _case_sel, _corrupt500, _row_map, _sel_host_decode, xtc_dir  # noqa: F401

pytestmark = pytest.mark.gpu

N_ATOMS, N_FRAMES, N_SEL = 3341, 31, 214


def _sel_device_decode(words, off, ln, n_atoms, sel, pad=0):
    """As test_xtc_select._sel_host_decode, through the kernel."""
    import torch

    from rmsf_amd._lib import call
    dev = torch.device("cuda")
    n, stride = len(off), 3 * len(sel) + pad
    d_words = torch.as_tensor(words.view(np.int32)).to(dev)
    d_off, d_ln = torch.as_tensor(off).to(dev), torch.as_tensor(ln).to(dev)
    d_map = torch.as_tensor(_row_map(sel, n_atoms)).to(dev)
    buf = torch.full((n + 1, stride), float(CANARY), dtype=torch.float32, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    call("rmsf_xtc_decode_records_sel", d_words.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), n, n_atoms,
         d_map.data_ptr(), len(sel), buf.data_ptr(), stride, st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("case,name", CASE_SEL)
def test_device_kernel_matches_host_twin(xtc_dir, case, name):  # noqa: F811
    _, words, off, ln, n_atoms, full, sel = _case_sel(case, name, xtc_dir)
    ref, st_ref = _sel_host_decode(words, off, ln, n_atoms, sel, pad=3)
    got, st = _sel_device_decode(words, off, ln, n_atoms, sel, pad=3)
    assert (st == 0).all() and (st_ref == 0).all()
    np.testing.assert_array_equal(got, ref)  # selected rows, padding and guard row alike
    np.testing.assert_array_equal(got[:-1, :3 * len(sel)].reshape(len(off), len(sel), 3), full[:, sel])
    assert (got[:-1, 3 * len(sel):] == CANARY).all() and (got[-1] == CANARY).all()


def test_device_kernel_corrupt_frames(tmp_path):
    """The three corruptions of test_corrupt_records_are_rejected and a frame
    whose stream breaks in pass 1: the host twin's statuses, NaN in the n_sel
    rows and nowhere else."""
    words, bad, off, ln, ln2, n_atoms = _corrupt500(tmp_path)
    sel = np.arange(3, n_atoms, 7, dtype=np.int32)[::-1].copy()
    _, st_full = _host_decode(bad, off, ln2, n_atoms)
    ref, st_ref = _sel_host_decode(bad, off, ln2, n_atoms, sel, pad=4)
    got, st = _sel_device_decode(bad, off, ln2, n_atoms, sel, pad=4)
    np.testing.assert_array_equal(st, st_ref)
    np.testing.assert_array_equal(st, st_full)
    assert (st != 0).all() and np.isnan(got[:-1, :3 * len(sel)]).all()
    assert (got[:-1, 3 * len(sel):] == CANARY).all() and (got[-1] == CANARY).all()
    # a garbage stream the decoders reject part-way (found on the host), beside two good frames
    rng = np.random.default_rng(0)
    g = None
    for t in range(60):
        g = words.copy()
        lo = off[1] + 24 + (t % 5) * 40
        g[lo:off[1] + ln[1]] = rng.integers(0, 2**32, off[1] + ln[1] - lo, dtype=np.uint64).astype(np.uint32)
        if _host_decode(g, off, ln, n_atoms)[1][1] != 0:
            break
    ref, st_ref = _sel_host_decode(g, off, ln, n_atoms, sel, pad=4)
    got, st = _sel_device_decode(g, off, ln, n_atoms, sel, pad=4)
    assert st_ref[1] != 0 and st_ref[0] == 0 and st_ref[2] == 0
    np.testing.assert_array_equal(st, st_ref)
    np.testing.assert_array_equal(got, ref)  # NaN == NaN positions: assert_array_equal treats them as equal


# -- the pinned-slot decoder -----------------------------------------------------

@pytest.fixture(scope="module")
def dec2000(tmp_path_factory):
    from rmsf_amd.xtc import XTCFile, write_xtc
    p = str(tmp_path_factory.mktemp("dec") / "t.xtc")
    write_xtc(p, _protein_like(np.random.default_rng(9), 2000, 12))
    with XTCFile(p) as f:
        ref = f.read()
    ref.setflags(write=False)
    return p, ref


def _d2h(ptr, shape, stream):
    from rmsf_amd._lib import call
    out = np.empty(shape, dtype=np.float32)
    call("rmsf_memcpy_d2h", out.ctypes.data, ptr, out.nbytes, stream)
    call("rmsf_stream_synchronize", stream)
    return out


def test_decoder_with_selection_bit_exact(dec2000):
    """decode (steps 1 and 3), decode_list, decode_into a strided buffer; 2
    slots x 8 frames, more batches than slots."""
    import torch

    from rmsf_amd import RmsfError
    from rmsf_amd.sources import XtcDecoder
    from rmsf_amd.xtc import XTCFile
    p, ref = dec2000
    sel = np.arange(0, 2000, 7)
    ns = len(sel)
    s = torch.cuda.current_stream().cuda_stream
    with XTCFile(p) as f:
        dec = XtcDecoder(f, batch_frames=8, n_slots=2, n_threads=4, sel=sel)
        assert dec.n_rows == ns
        for step in (1, 3):
            for first in range(0, 12, 8 * step):  # step 1: two batches
                n = len(range(first, 12, step)[:8])
                slot, ptr = dec.decode(first, n, step, s)
                np.testing.assert_array_equal(_d2h(ptr, (n, ns, 3), s), ref[first:first + n * step:step][:, sel])
                dec.release(slot, s)
        for _ in range(3):  # more batches than slots
            lst = np.array([7, 1, 1, 11, 0, 4], dtype=np.int64)
            slot, ptr = dec.decode_list(lst, s)
            np.testing.assert_array_equal(_d2h(ptr, (len(lst), ns, 3), s), ref[lst][:, sel])
            dec.release(slot, s)
        pitch = 3 * ns + 7
        buf = torch.full((5, pitch), float(CANARY), dtype=torch.float32, device="cuda")
        slot = dec.decode_into(2, 4, 3, buf.data_ptr(), pitch, s)
        dec.synchronize()
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        np.testing.assert_array_equal(got[:4, :3 * ns].reshape(4, ns, 3), ref[2:12:3][:, sel])
        assert (got[:4, 3 * ns:] == CANARY).all() and (got[4] == CANARY).all()
        dec.release(slot, s)
        with pytest.raises(RmsfError):  # the stride check is against 3 n_sel
            dec.decode_into(0, 1, 1, buf.data_ptr(), 3 * ns - 1, s)
        dec.synchronize()
        dec.close()


def test_decoder_create_sel_rejects_bad_selections(dec2000):
    from rmsf_amd import RmsfError
    from rmsf_amd.sources import XtcDecoder
    from rmsf_amd.xtc import XTCFile
    with XTCFile(dec2000[0]) as f:
        with pytest.raises(RmsfError, match="twice"):
            XtcDecoder(f, 4, sel=[5, 9, 5])
        with pytest.raises(RmsfError, match="out of range"):
            XtcDecoder(f, 4, sel=[5, 2000])
        with pytest.raises(RmsfError, match="out of range"):
            XtcDecoder(f, 4, sel=[-1])


# -- XtcSource -----------------------------------------------------------------

@pytest.fixture(scope="module")
def traj31(tmp_path_factory):
    """3,341 atoms x 31 frames, 214 sorted random atoms; the host-decoded frames."""
    from rmsf_amd.xtc import XTCFile, write_xtc
    p = str(tmp_path_factory.mktemp("src") / "t.xtc")
    write_xtc(p, _protein_like(np.random.default_rng(8), N_ATOMS, N_FRAMES))
    sel = np.sort(np.random.default_rng(2).choice(N_ATOMS, N_SEL, replace=False))
    with XTCFile(p) as f:
        dec = f.read()
    dec.setflags(write=False)
    return p, sel, dec


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("align", [None, "frame0", "average"])
def test_source_selected_decode_equals_host_decode(traj31, align, step):
    from oracle import rmsf_oracle as O
    from rmsf_amd import RMSF
    from rmsf_amd.sources import XtcSource
    p, sel, dec = traj31
    src = XtcSource(p, sel, batch_frames=5, decode_select=True)
    assert src.decode_select and src.sel_dev is None
    got = RMSF(src, align=align).run(step=step).results
    host = RMSF(XtcSource(p, sel, batch_frames=5, decode="host"), align=align).run(step=step).results
    np.testing.assert_array_equal(got.rmsf, host.rmsf)  # compact batches, the same splits
    assert ("average" in got) == (align == "average")  # the results carry it for the two-sweep run only
    if align == "average":
        np.testing.assert_array_equal(got.average, host.average)
    exp = O.rmsf_script(dec, sel, None, size=1, align=align, start=0, stop=N_FRAMES, step=step)["rmsf"]
    np.testing.assert_allclose(got.rmsf, exp, rtol=0, atol=1e-6)
    # exact=True: RMSF.py's own order of operations, whichever way the atoms arrive
    a = RMSF(XtcSource(p, sel, batch_frames=5, decode_select=True), align=align, exact=True).run(step=step).results
    b = RMSF(XtcSource(p, sel, batch_frames=5, decode_select=False), align=align, exact=True).run(step=step).results
    np.testing.assert_array_equal(a.rmsf, b.rmsf)


def test_source_decode_select_default(traj31):
    """None = on for a proper subset with unique indices; off otherwise."""
    from rmsf_amd.sources import XtcSource
    p, sel, _ = traj31
    assert XtcSource(p, sel).decode_select
    assert not XtcSource(p, None).decode_select
    assert not XtcSource(p, np.array([4, 9, 4])).decode_select
    assert not XtcSource(p, np.arange(N_ATOMS)[::-1]).decode_select
    assert not XtcSource(p, sel, decode="host").decode_select
    assert not XtcSource(p, sel, decode_select=False).decode_select
    assert XtcSource(p, np.arange(N_ATOMS)[::-1], decode_select=True).decode_select


def _count_decodes(monkeypatch):
    from rmsf_amd.sources import XtcDecoder
    calls = []
    for name in ("decode", "decode_into", "decode_list"):
        orig = getattr(XtcDecoder, name)

        def wrap(self, *a, _orig=orig, _name=name):
            calls.append(_name)
            return _orig(self, *a)

        monkeypatch.setattr(XtcDecoder, name, wrap)
    return calls


@pytest.mark.parametrize("step", [1, 3])
def test_selected_cache_two_sweeps(traj31, monkeypatch, step):
    from rmsf_amd import RMSF
    from rmsf_amd.sources import XtcSource
    p, sel, _ = traj31
    calls = _count_decodes(monkeypatch)
    src = XtcSource(p, sel, batch_frames=5, cache=True, decode_select=True)
    assert src.cache is not None and tuple(src.cache.shape) == (N_FRAMES, N_SEL, 3)
    a = RMSF(src, align="average").run(step=step).results
    assert src._cached[::step].all() and len(calls) > 0
    n_first = len(calls)
    b = RMSF(src, align="average").run(step=step).results  # every frame from HBM
    assert len(calls) == n_first
    np.testing.assert_array_equal(a.rmsf, b.rmsf)
    np.testing.assert_array_equal(a.average, b.average)
    host = RMSF(XtcSource(p, sel, batch_frames=5, decode="host"), align="average").run(step=step).results
    np.testing.assert_array_equal(a.rmsf, host.rmsf)
    src.drop_cache()
    assert not src._cached.any()
    c = RMSF(src, align="average").run(step=step).results  # decodes again
    assert len(calls) > n_first
    np.testing.assert_array_equal(a.rmsf, c.rmsf)


@pytest.mark.parametrize("cache", [False, True])
@pytest.mark.parametrize("align", [None, "average"])
def test_selected_scattered_frames(tmp_path, cache, align):
    """The frame list of test_scattered_frames_batched_decode (which shows why
    list batches and runs are equal to rounding only, not bit for bit)."""
    from oracle import rmsf_oracle as O
    from rmsf_amd import RMSF
    from rmsf_amd.sources import XtcSource
    from rmsf_amd.xtc import XTCFile, write_xtc
    p = str(tmp_path / "t.xtc")
    write_xtc(p, _protein_like(np.random.default_rng(6), 1500, 40))
    sel = np.arange(0, 1500, 3)
    idx = np.array([0, 2, 3, 9, 10, 17, 18, 25, 31, 33, 38])
    src = XtcSource(p, sel, batch_frames=4, cache=cache, decode_select=True)
    got = RMSF(src, align=align).run(frames=idx).results.rmsf
    if cache:
        assert src._cached[idx].all() and tuple(src.cache.shape) == (40, len(sel), 3)
        again = RMSF(src, align=align).run(frames=idx).results.rmsf  # gathered from the cache
        np.testing.assert_allclose(again, got, rtol=0, atol=1e-12)
    host = RMSF(XtcSource(p, sel, batch_frames=4, decode="host"), align=align).run(frames=idx).results.rmsf
    np.testing.assert_allclose(got, host, rtol=0, atol=1e-12)
    with XTCFile(p) as f:
        dec = f.read()
    exp = O.rmsf_script(dec[idx], sel, None, size=1, align=align)["rmsf"]
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-6)


def test_selected_cache_fits_where_whole_frames_do_not(traj31, monkeypatch):
    """Free memory of 4x the selected cache at a 1-in-10 selection: whole
    frames (10x) are refused, the selected rows are cached; same RMSF."""
    import torch

    from rmsf_amd import RMSF
    from rmsf_amd.sources import XtcSource
    p, _, _ = traj31
    sel = np.arange(0, N_ATOMS, 10)
    need = 12 * N_FRAMES * len(sel)
    total = torch.cuda.mem_get_info()[1]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (4 * need, total))
    whole = XtcSource(p, sel, batch_frames=5, cache=True, decode_select=False)
    picked = XtcSource(p, sel, batch_frames=5, cache=True, decode_select=True)
    assert whole.cache is None
    assert picked.cache is not None and picked.cache.numel() * 4 == need
    a = RMSF(whole, align="average").run().results.rmsf
    b = RMSF(picked, align="average").run().results.rmsf
    np.testing.assert_array_equal(a, b)


def test_selected_cache_forgets_corrupt_frames(tmp_path):
    from rmsf_amd import RMSF, RmsfError
    from rmsf_amd.sources import XtcSource
    from rmsf_amd.xtc import write_xtc
    p = str(tmp_path / "t.xtc")
    write_xtc(p, _protein_like(np.random.default_rng(4), 500, 6))
    words, off, _, _ = _records(p)
    words = words.copy()
    words[off[3] + 14 + 7] = np.array([200], ">u4").view(np.uint32)[0]  # frame 3: smallidx out of the table
    words.tofile(p)
    src = XtcSource(p, np.arange(1, 500, 5), cache=True, batch_frames=2)
    assert src.decode_select
    with pytest.raises(RmsfError, match="frame 3"):
        RMSF(src, align="average").run()
    assert not src._cached.any()


# -- the context ---------------------------------------------------------------

@pytest.mark.parametrize("frames", [None, [0, 2, 3, 9, 10, 17, 18, 25, 30]])
def test_context_push_xtc_decodes_the_selection(traj31, frames):
    """rmsf_push_xtc / rmsf_push_xtc_frames on a context with the 214-atom
    selection: the bits of pushing the host-decoded selected frames."""
    from rmsf_amd.context import PUSH_ALIGN_SUM, PUSH_ALIGN_WELFORD, PUSH_WELFORD, Context
    from rmsf_amd.xtc import XTCFile
    p, sel, dec = traj31
    picked = np.ascontiguousarray(dec[:, sel] if frames is None else dec[frames][:, sel])
    with XTCFile(p) as x, Context(N_ATOMS, sel=sel) as a, Context(N_SEL) as b:
        def push_a(mode):
            if frames is None:
                a.push_xtc(x, 0, None, 1, mode)
            else:
                a.push_xtc_frames(x, frames, mode)

        push_a(PUSH_WELFORD)
        b.push(picked, PUSH_WELFORD)
        np.testing.assert_array_equal(a.rmsf(), b.rmsf())
        a.reset()
        b.reset()
        a.set_reference_frame(dec[0])
        b.set_reference_frame(np.ascontiguousarray(dec[0][sel]))
        push_a(PUSH_ALIGN_SUM)
        b.push(picked, PUSH_ALIGN_SUM)
        for c in (a, b):
            c.allreduce_sum()
            c.set_reference_average()
        push_a(PUSH_ALIGN_WELFORD)
        b.push(picked, PUSH_ALIGN_WELFORD)
        np.testing.assert_array_equal(a.average(), b.average())
        np.testing.assert_array_equal(a.rmsf(), b.rmsf())
