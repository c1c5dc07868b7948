"""GPU tier of ``DiffusionMap(solver="device")``: the kernel pass and the row
scaling of csrc/diffusion.hip against numpy on the same bits, then the public
class from a matrix, from a trajectory and from the caller's HBM tensor against
the host path.

Bounds (derived, not measured):
  * kernel pass, results that are normal f64 numbers: 4 ulp -- the argument
    -(d d) / epsilon has numpy's bits, both exponentials are documented to about
    1 ulp, so they differ by at most 2, and the bound doubles that; below
    2^-1022: 4 2^-1074 absolute.  Row sums: n 2^-52 relative to ``numpy.sum``
    of the device's K -- two sums of n positive terms, (n - 1) 2^-53 each.
  * ``scale_rows``: one multiply an element, numpy's bits.
  * end to end: the driver stops at a residual of 1e-10 lambda_1 = 1e-10, the
    kernel's ulps add about 1e-15: eigenvalues, the constant vector and the
    conjugate residual to 1e-9, ten times the rule; eigenvectors to 1e-9 / gap
    (Davis-Kahan), the gap from the host spectrum.  The vectors compared are
    P's right eigenvectors t v with t = rowsum^-1/2 <= 1 (the diagonal of K is
    1), so the bound of the orthonormal v holds for them.

The cases are tests/diffusion_cases.py's; tests/test_diffusion_host.py asserts
on the CPU that the driver converges on them in under 50 iterations and that
their first eigenvalues are at least 1e-3 apart (0.02 at the least)."""
import functools

import numpy as np
import pytest

import diffusion_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77
EPSILON = 2.0
TINY = 2.0 ** -1022


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64)


def engine():
    import torch

    from rmsf_amd.engine import Engine
    return Engine(torch.device("cuda", 0))


# ---- 1. the kernel pass ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seeded_distances(n: int):
    """(symmetric f64 [n, n] with a zero diagonal, the planted pairs): most
    distances uniform in [0, 3), one in ten in [0, 40) -- with EPSILON = 2 the
    arguments reach -800, through the subnormal results to the underflow --
    and, where n has room, a zero pair, a pair with d^2 / epsilon > 800 and a
    +inf pair."""
    rng = np.random.default_rng(n)
    d = np.where(rng.random((n, n)) < 0.1, rng.uniform(0.0, 40.0, (n, n)), rng.uniform(0.0, 3.0, (n, n)))
    d = np.triu(d, 1)
    d = d + d.T
    pairs = {}
    if n >= 8:
        pairs = {"zero": (1, 5), "under": (0, 3), "inf": (2, 7)}
        for name, v in (("zero", 0.0), ("under", np.sqrt(800.0 * EPSILON) * 1.001), ("inf", np.inf)):
            i, j = pairs[name]
            d[i, j] = d[j, i] = v
        assert d[0, 3] ** 2 / EPSILON > 800.0
    d.setflags(write=False)
    return d, pairs


def device_pass(eng, d: np.ndarray, pad: int, eps: float = EPSILON):
    """rmsf_diffusion_kernel on ``d`` in a [n, n + pad] buffer of sentinels ->
    (the whole buffer, the row sums), host arrays."""
    import torch
    n = d.shape[0]
    buf = torch.full((n, n + pad), SENTINEL, dtype=torch.float64, device="cuda:0")
    buf[:, :n] = torch.tensor(d, device="cuda:0")
    rs = eng.diffusion_kernel(buf, eps, n)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), rs.cpu().numpy()


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 353, 1100, 2050, 2051])
def test_kernel_pass(n, pad):
    """Up to 353 every element goes through the single-step loops.  The
    unrolled loops take 4 x 256 accesses a turn: 1100 enters the 8-byte one
    (ld = 1105, odd), 2050 and 2051 the 8-byte one (ld = 2055 and 2051) and the
    16-byte one (1,025 pairs: one turn, one pair left, and at 2051 the odd last
    element; ld = 2050 and 2056)."""
    eng = engine()
    d, pairs = seeded_distances(n)
    buf, rs = device_pass(eng, d, pad)
    got = buf[:, :n]
    assert np.all(buf[:, n:] == SENTINEL)                          # the padding is not written
    with np.errstate(over="ignore", under="ignore"):
        want = np.exp(-(d * d) / EPSILON)
    assert np.all(np.isfinite(got))
    normal = want >= TINY
    ulps = np.abs(got - want)[normal] / np.spacing(want[normal])
    print(f"n {n} ld {n + pad}: worst {ulps.max()} ulp over {normal.sum()} normal results, "
          f"{(~normal & (want > 0)).sum()} subnormal, {(want == 0).sum()} zero")
    assert ulps.max() <= 4.0
    assert np.all(np.abs(got - want)[~normal] <= 4 * 2.0 ** -1074)
    for name in ("under", "inf"):
        if name in pairs:
            i, j = pairs[name]
            assert bits(got[i, j]) == bits(got[j, i]) == bits(0.0), name           # exactly +0, never NaN
    if pairs:
        assert got[pairs["zero"]] == 1.0
    assert np.array_equal(bits(got), bits(got.T))                  # symmetric in its bits
    assert np.all(np.diagonal(got) == 1.0)
    ref = got.sum(axis=1)
    assert np.all(np.abs(rs - ref) <= n * 2.0 ** -52 * ref)
    buf2, rs2 = device_pass(eng, d, pad)                           # a second run: the same bits
    assert np.array_equal(bits(buf2), bits(buf)) and np.array_equal(bits(rs2), bits(rs))


@pytest.mark.parametrize("pad", [0, 5])
def test_kernel_pass_nan_entry_reaches_its_two_row_sums_only(pad):
    eng = engine()
    d, _ = seeded_distances(65)
    _, rs = device_pass(eng, d, pad)
    bad = np.array(d)
    bad[4, 40] = bad[40, 4] = np.nan
    buf, rs_bad = device_pass(eng, bad, pad)
    assert np.isnan(buf[4, 40]) and np.isnan(buf[40, 4]) and np.isnan(buf[:, :65]).sum() == 2
    assert np.isnan(rs_bad[4]) and np.isnan(rs_bad[40])
    rest = np.setdiff1d(np.arange(65), [4, 40])
    assert np.array_equal(bits(rs_bad[rest]), bits(rs[rest]))


def test_kernel_pass_bad_arguments():
    import torch

    from rmsf_amd._lib import RMSF_EINVAL
    eng = engine()
    m, rs = eng.zeros(8, 8), eng.zeros(8)
    p, q = m.data_ptr(), rs.data_ptr()
    for args in [(None, 8, 8, 1.0, q, None), (p, 8, 8, 1.0, None, None), (p, 8, 0, 1.0, q, None),
                 (p, 7, 8, 1.0, q, None), (p, 8, 8, 0.0, q, None), (p, 8, 8, -2.0, q, None),
                 (p, 8, 8, float("inf"), q, None), (p, 8, 8, float("nan"), q, None)]:
        assert eng.lib.rmsf_diffusion_kernel(*args) == RMSF_EINVAL, args
        assert b"rmsf_diffusion_kernel" in eng.lib.rmsf_last_error()
    a = eng.zeros(8, 8)
    s, pa = rs.data_ptr(), a.data_ptr()
    for args in [(None, pa, 8, 8, 8, p, 8, None), (s, None, 8, 8, 8, p, 8, None), (s, pa, 8, 8, 8, None, 8, None),
                 (s, pa, 8, 0, 8, p, 8, None), (s, pa, 8, 8, 0, p, 8, None), (s, pa, 49, 8, 49, p, 49, None),
                 (s, pa, 7, 8, 8, p, 8, None), (s, pa, 8, 8, 8, p, 7, None)]:
        assert eng.lib.rmsf_block_scale_rows(*args) == RMSF_EINVAL, args
        assert b"rmsf_block_scale_rows" in eng.lib.rmsf_last_error()
    torch.cuda.synchronize()
    assert float(m.abs().sum()) == 0.0 and float(rs.abs().sum()) == 0.0       # nothing was launched
    with pytest.raises(ValueError):
        eng.diffusion_kernel(m.to(torch.float32), 1.0)
    with pytest.raises(ValueError):
        eng.block_scale_rows(rs[:7], a, 8, 8, m)


# ---- 2. scale_rows -----------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("cols", [1, 17, 48])
def test_scale_rows(cols, in_place):
    import torch
    n = 49
    eng = engine()
    rng = np.random.default_rng(cols)
    s, a = rng.standard_normal(n), rng.standard_normal((n, cols))
    sd = torch.tensor(s, device="cuda:0")
    ad = torch.full((n, cols + 3), SENTINEL, dtype=torch.float64, device="cuda:0")
    ad[:, :cols] = torch.tensor(a, device="cuda:0")
    cd = ad if in_place else torch.full((n, cols + 2), SENTINEL, dtype=torch.float64, device="cuda:0")
    eng.block_scale_rows(sd, ad, n, cols, cd)
    torch.cuda.synchronize()
    c = cd.cpu().numpy()
    assert np.array_equal(bits(c[:, :cols]), bits(s[:, None] * a))
    assert np.all(c[:, cols:] == SENTINEL)
    if not in_place:
        assert np.array_equal(bits(ad.cpu().numpy()[:, :cols]), bits(a))


# ---- 3. end to end -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_case(kind: str, n: int):
    """(DistanceMatrix's host matrix of the planted trajectory, epsilon, the
    host path on it as ``diffusion_cases.host_formulae`` returns it, the host
    ``transform(2, 1.0)``)."""
    import torch

    from rmsf_amd import DiffusionMap, DistanceMatrix
    d = DistanceMatrix(torch.tensor(C.planted(kind, n), device="cuda:0")).run().results.dist_matrix
    d.setflags(write=False)
    eps = C.epsilon_of(kind, d)
    ref = C.host_formulae(d, eps)
    host = DiffusionMap(d, epsilon=eps).run()
    assert np.array_equal(bits(host.results.eigenvalues), bits(ref[0]))
    assert np.array_equal(bits(host.results.eigenvectors), bits(ref[1]))
    return d, eps, ref, host.transform(2, 1.0)


def check_against_host(dm, kind: str, n: int, label: str):
    d, eps, (w, right, sym, rs, v), host_t = host_case(kind, n)
    r, k = dm.results, C.K + 1
    lam, vec = r.eigenvalues, r.eigenvectors
    assert lam.shape == (k,) and vec.shape == (n, k) and vec.dtype == np.float64 and r.n_frames == n
    info = r.solver_info
    assert info["converged"] and info["n_iter"] < 50
    gaps = -np.diff(w[:k + 1])
    assert gaps.min() >= 1e-3
    conj = vec / rs[:, None]                                       # the conjugate's vectors, from the host's row sums
    res = np.linalg.norm(sym @ conj - conj * lam, axis=0)
    const = np.abs(vec[:, 0] - vec[:, 0].mean()).max() / abs(vec[:, 0].mean())
    dv = np.linalg.norm(C.aligned(vec, right[:, :k]) - right[:, :k], axis=0)
    bound = 1e-9 / np.array([gaps[0]] + [min(gaps[i - 1], gaps[i]) for i in range(1, k)])
    t = dm.transform(2, 1.0)
    dt = np.linalg.norm(C.aligned(t, host_t) - host_t, axis=0)
    print(f"{label} {kind} {n}: {info['n_iter']} iterations, max |dlambda| {np.abs(lam - w[:k]).max():.3e}, "
          f"|lambda_1 - 1| {abs(lam[0] - 1):.3e}, constant to {const:.3e}, residual {res.max():.3e}, "
          f"max |dv| x gap {(dv / bound).max() * 1e-9:.3e}, max |dtransform| x gap {(dt / bound[1:3]).max() * 1e-9:.3e}")
    assert np.all(np.diff(lam) <= 0)
    assert np.abs(lam - w[:k]).max() <= 1e-9
    assert abs(lam[0] - 1.0) <= 1e-9
    assert const <= 1e-9 and np.all(vec[:, 0] > 0)
    assert res.max() <= 1e-9
    assert np.all(dv <= bound)
    assert t.shape == (n, 2) and np.all(dt <= bound[1:3])          # lambda <= 1 scales the error down
    with pytest.raises(ValueError, match=f"1..{C.K}"):
        dm.transform(C.K + 1, 1.0)


@pytest.mark.parametrize("kind,n", C.CASES)
def test_device_solver_from_a_matrix(kind, n):
    import torch

    from rmsf_amd import DiffusionMap, DistanceMatrix
    d, eps = host_case(kind, n)[:2]
    check_against_host(DiffusionMap(np.array(d), epsilon=eps, n_eigenvectors=C.K, solver="device").run(), kind, n,
                       "host array")
    if (kind, n) == C.CASES[0]:                                    # a DistanceMatrix that has run: its host matrix
        ran = DistanceMatrix(torch.tensor(C.planted(kind, n), device="cuda:0")).run()
        check_against_host(DiffusionMap(ran, epsilon=eps, n_eigenvectors=C.K, solver="device").run(), kind, n,
                           "run DistanceMatrix")


@pytest.mark.parametrize("kind,n", C.CASES[:2])
@pytest.mark.parametrize("where", ["hbm", "host"])
def test_device_solver_from_a_trajectory(kind, n, where):
    import torch

    from rmsf_amd import DiffusionMap, DistanceMatrix
    eps = host_case(kind, n)[1]
    x = C.planted(kind, n)
    inner = DistanceMatrix(torch.tensor(x, device="cuda:0") if where == "hbm" else np.array(x))
    dm = DiffusionMap(inner, epsilon=eps, n_eigenvectors=C.K, solver="device").run()
    check_against_host(dm, kind, n, f"{where} trajectory")
    assert inner.results.get("dist_matrix") is None                # nothing went through the host
    assert inner.n_frames == n and np.array_equal(inner.results.frames, np.arange(n))


def test_device_solver_leaves_the_caller_s_tensor():
    import torch

    from rmsf_amd import DiffusionMap
    kind, n = C.CASES[0]
    d, eps = host_case(kind, n)[:2]
    mine = torch.tensor(d, device="cuda:0")
    check_against_host(DiffusionMap(mine, epsilon=eps, n_eigenvectors=C.K, solver="device").run(), kind, n,
                       "HBM tensor")
    assert np.array_equal(bits(mine.cpu().numpy()), bits(d))
    wide = torch.full((n, n + 3), SENTINEL, dtype=torch.float64, device="cuda:0")     # a view with wider rows
    wide[:, :n] = mine
    check_against_host(DiffusionMap(wide[:, :n], epsilon=eps, n_eigenvectors=C.K, solver="device").run(), kind, n,
                       "HBM view")
    assert np.array_equal(bits(wide.cpu().numpy()[:, :n]), bits(d))


def test_device_solver_errors():
    import torch

    from rmsf_amd import DiffusionMap, DistanceMatrix
    x = np.array(C.planted("states", 130))
    x[17, 5, 1] = np.nan                                           # a NaN frame: a NaN row and column
    with pytest.raises(ValueError, match="the distance matrix has non-finite entries"):
        DiffusionMap(DistanceMatrix(torch.tensor(x, device="cuda:0")), epsilon=3.0, n_eigenvectors=3,
                     solver="device").run()
    far = np.full((6, 6), 100.0)                                   # every row sum underflows to 0
    with pytest.raises(ValueError, match="the distance matrix has non-finite entries"):
        DiffusionMap(far, epsilon=1.0, n_eigenvectors=3, solver="device").run()
    d30 = np.array(host_case("states", 130)[0][:30, :30])
    with pytest.raises(ValueError, match="n_eigenvectors = 39 .* 30 frames: ask for at most 29") as e:
        DiffusionMap(d30, epsilon=3.0, n_eigenvectors=39, solver="device").run()
    assert "at most min(40, n = 30) components" in str(e.value.__cause__)      # block_width: k + 1 = 40 > F = 30
    short = DistanceMatrix(torch.tensor(C.planted("states", 130)[:30], device="cuda:0"))
    with pytest.raises(ValueError, match="ask for at most 29"):    # a trajectory: refused before its matrix is computed
        DiffusionMap(short, epsilon=3.0, n_eigenvectors=39, solver="device").run()
    assert short.n_frames == 30 and short.results.get("dist_matrix") is None
    lop = np.array(host_case("states", 130)[0])
    assert lop[2, 7] > 0.1
    lop[2, 7] *= 1.0 + 1e-12                                       # off its mirror by a few thousand ulp
    for inp in (lop, torch.tensor(lop, device="cuda:0")):
        with pytest.raises(ValueError, match="exactly symmetric"):
            DiffusionMap(inp, epsilon=3.0, n_eigenvectors=3, solver="device").run()
    assert DiffusionMap(lop, epsilon=3.0).run().results.eigenvalues.shape == (130,)     # the host path forgives it
    with pytest.raises(ValueError, match="square"):
        DiffusionMap(np.zeros((3, 4)), n_eigenvectors=1, solver="device").run()
    with pytest.raises(ValueError, match="float64"):
        DiffusionMap(torch.zeros((4, 4), device="cuda:0"), n_eigenvectors=1, solver="device").run()


def test_script_writes_the_embedding(tmp_path):
    """rmsf_mi355x.py --diffusion-map beside --dist-matrix: the host path's
    ``transform(2, 1)`` of the matrix it writes.  The synthetic trajectory is
    noise about one structure, a flat spectrum behind the constant mode: at
    epsilon = 8 A^2 (its median d^2 is 8.27) the CPU twin needs 46 iterations
    for k = 2 and the first three gaps are 0.92, 6.4e-3 and 2.0e-3."""
    import subprocess
    import sys

    from conftest import ROOT
    from rmsf_amd import DiffusionMap
    n_atoms, n_frames, eps = 64, 40, 8.0
    out, dm = str(tmp_path / "embedding.npy"), str(tmp_path / "dm.npy")
    r = subprocess.run([sys.executable, f"{ROOT}/mdanalysis-mpi_amd/rmsf_mi355x.py", "--synthetic", str(n_atoms),
                        str(n_frames), "--align", "average", "--dist-matrix", dm, "--diffusion-map", out,
                        "--diffusion-epsilon", repr(eps), "--n-eigenvectors", "2"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    emb = np.load(out)
    host = DiffusionMap(np.load(dm), epsilon=eps).run()
    want, w = host.transform(2, 1.0), host.results.eigenvalues
    gaps = -np.diff(w[:4])
    assert emb.shape == (n_frames, 2) and emb.dtype == np.float64 and gaps.min() >= 1e-3
    bound = 1e-9 / np.minimum(gaps[:2], gaps[1:3])
    assert np.all(np.linalg.norm(C.aligned(emb, want) - want, axis=0) <= bound)
