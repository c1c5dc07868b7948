"""CPU tier: the lambda of the RMSD matrices' epilogue (``pair_lambda`` of
csrc/rmsf_device.h) run on the host through ``rmsf_pair_lambda_host`` -- the
function ``pair_epilogue`` / ``cross_epilogue`` of csrc/pairwise.hip call on
the device -- on the pairs of tests/pairwise_zoo.py and on 2,000 generic pairs.

  * accuracy: ``|2 (E0 - lambda) / N - d^2_ref| <= 1e-12 E0 / N`` on every pair,
    ``d^2_ref`` from numpy's SVD of the same 3 x 3 matrix;
  * generic pairs take the Newton path and give qcprot's bits (the oracle's
    ``rmsd``);
  * the tests bite: qcprot's Newton iteration alone (the oracle's, the
    epilogue before the Jacobi fallback) misses that bound by 100 x or more on
    each flagged degenerate family.
"""
import ctypes

import numpy as np
import pytest

import pairwise_zoo as Z

BOUND = 1e-12


def pair_lambda(a: np.ndarray, e0: np.ndarray):
    """(lambda [n], path [n]) of a [n, 9], e0 [n]."""
    from rmsf_amd import _lib
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 9)
    e0 = np.ascontiguousarray(e0, dtype=np.float64).reshape(-1)
    assert len(a) == len(e0)
    lam = np.full(len(e0), -1.0)
    path = np.full(len(e0), -1, dtype=np.int32)
    _lib.call("rmsf_pair_lambda_host", a.ctypes.data, e0.ctypes.data, len(e0), lam.ctypes.data, path.ctypes.data)
    return lam, path


def oracle_rmsd(a: np.ndarray, e0: np.ndarray, n: float):
    """(rmsd [n], Newton steps [n]) of qcprot's arithmetic, restated in
    oracle.rmsf_oracle."""
    from oracle.rmsf_oracle import fast_calc_rmsd_and_rotation
    out = [fast_calc_rmsd_and_rotation(ai, float(ei), n)[1:] for ai, ei in zip(a.reshape(-1, 9), e0.reshape(-1))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def ratios(d2: np.ndarray, a: np.ndarray, e0: np.ndarray, n: float) -> np.ndarray:
    """|d2 - d2_ref| / (1e-12 E0 / N); 0 where both sides are 0."""
    err = np.abs(d2 - Z.svd_sq(a, e0, n).reshape(-1))
    bound = BOUND * e0.reshape(-1) / n
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((err == 0.0) & (bound == 0.0), 0.0, err / bound)


def generic_pairs(count=2000, n=40):
    """Two conformations of one structure, as the frames of a trajectory are:
    a random structure of 40 atoms, and it displaced by 1 A per coordinate and
    rotated at random."""
    rng = np.random.default_rng(11)
    base = rng.normal(scale=6.0, size=(count, n, 3))
    moved = np.einsum("kac,kcd->kad", base + rng.normal(size=(count, n, 3)),
                      np.stack([Z.rotation(rng) for _ in range(count)]))
    x = np.stack([base, moved]).astype(np.float32).astype(np.float64)
    x -= x.mean(axis=2, keepdims=True)
    a = np.einsum("kac,kad->kcd", x[0], x[1]).reshape(count, 9)
    e0 = 0.5 * ((x[0] ** 2).sum(axis=(1, 2)) + (x[1] ** 2).sum(axis=(1, 2)))
    return a, e0, float(n)


def zoo_pairs(n_sel: int, weighted: bool):
    """Every pair of the 20-frame zoo: (A [20, 20, 9], E0 [20, 20], sum w)."""
    x = Z.zoo(20, n_sel, False)
    return Z.pair_inputs(x, x, Z.weights_of(n_sel) if weighted else None)


def flagged(n_sel: int, weighted: bool):
    """(family, A [k, 9], E0 [k], sum w) of each flagged family."""
    a, e0, wt = zoo_pairs(n_sel, weighted)
    for family, first, others in Z.FLAGGED:
        i = Z.index_of(20, first)
        js = [Z.index_of(20, o) for o in others]
        yield family, a[i, js], e0[i, js], wt
    x = Z.few_atoms(17, 2, False)
    a2, e2, wt2 = Z.pair_inputs(x, x, Z.weights_of(2) if weighted else None)
    off = ~np.eye(17, dtype=bool)
    yield "two atoms", a2[off], e2[off], wt2


def test_entry_point_and_its_argument_checks():
    from rmsf_amd import _lib
    lib = _lib.load()
    assert "rmsf_pair_lambda_host" in _lib.SIGNATURES and hasattr(lib, "rmsf_pair_lambda_host")
    one = ctypes.c_void_p(16)     # never dereferenced: the checks fail first
    for args in ((None, one, 1, one, None), (one, None, 1, one, None), (one, one, 1, None, None),
                 (one, one, -1, one, None)):
        assert lib.rmsf_pair_lambda_host(*args) == _lib.RMSF_EINVAL
        assert b"rmsf_pair_lambda_host" in lib.rmsf_last_error()
    assert lib.rmsf_pair_lambda_host(one, one, 0, one, None) == _lib.RMSF_OK
    # the path is optional; two all-zero frames: lambda = E0 = 0; a NaN stays one
    a = np.zeros((3, 9))
    a[1] = np.eye(3).reshape(9)
    e0 = np.array([0.0, 3.0, np.nan])
    lam = np.empty(3)
    assert lib.rmsf_pair_lambda_host(a.ctypes.data, e0.ctypes.data, 3, lam.ctypes.data, None) == _lib.RMSF_OK
    lam2, path = pair_lambda(a, e0)
    assert np.array_equal(lam.view(np.uint64), lam2.view(np.uint64))
    assert lam[0] == 0.0 and abs(lam[1] - 3.0) <= 1e-14 and np.isnan(lam[2])
    assert list(path) == [_lib.RMSF_PAIR_ZERO, _lib.RMSF_PAIR_NEWTON, _lib.RMSF_PAIR_ZERO]
    # a NaN in A alone comes out too
    a[1, 4] = np.nan
    assert np.isnan(pair_lambda(a, e0)[0][1])


def test_generic_pairs_keep_the_newton_path_and_qcprot_bits():
    from rmsf_amd import _lib
    a, e0, n = generic_pairs()
    lam, path = pair_lambda(a, e0)
    assert np.all(path == _lib.RMSF_PAIR_NEWTON)
    rmsd, steps = oracle_rmsd(a, e0, n)
    assert steps.max() <= 6, steps.max()
    got = np.sqrt(np.abs(2.0 * (e0 - lam) / n))
    assert np.array_equal(got.view(np.uint64), rmsd.view(np.uint64))
    r = ratios(2.0 * (e0 - lam) / n, a, e0, n)
    print(f"generic: max ratio {r.max():.3e}")
    assert r.max() <= 1.0


def test_mirror_images_keep_the_newton_path():
    """A generic frame against its point reflection: 9 steps, still exact."""
    from rmsf_amd import _lib
    for n_sel in (8, 40):
        a, e0, wt = zoo_pairs(n_sel, False)
        i, j = Z.index_of(20, "G"), Z.index_of(20, "mG")
        lam, path = pair_lambda(a[i, j], e0[i, j])
        assert path[0] == _lib.RMSF_PAIR_NEWTON
        rmsd, _ = oracle_rmsd(a[i, j], e0[i, j], wt)
        got = np.sqrt(np.abs(2.0 * (e0[i, j] - lam) / wt))
        assert np.array_equal(got.view(np.uint64), rmsd.view(np.uint64))


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("n_sel", [8, 40])
def test_every_zoo_pair_is_inside_the_bound(n_sel, weighted):
    from rmsf_amd import _lib
    a, e0, wt = zoo_pairs(n_sel, weighted)
    lam, path = pair_lambda(a, e0)
    assert set(path) <= {_lib.RMSF_PAIR_NEWTON, _lib.RMSF_PAIR_JACOBI, _lib.RMSF_PAIR_ZERO}
    assert not np.isnan(lam).any()
    r = ratios(2.0 * (e0.reshape(-1) - lam) / wt, a, e0, wt)
    print(f"zoo n_sel={n_sel} weighted={weighted}: max ratio {r.max():.3e}, "
          f"{int((path == _lib.RMSF_PAIR_JACOBI).sum())} of {len(path)} pairs by Jacobi")
    assert r.max() <= 1.0
    # the two all-zero frames: lambda = E0 = 0 exactly
    z = Z.index_of(20, "Z0") * 20 + Z.index_of(20, "Z1")
    assert lam[z] == 0.0 and e0.reshape(-1)[z] == 0.0 and path[z] == _lib.RMSF_PAIR_ZERO


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("n_sel", [8, 40])
def test_flagged_families_are_degenerate_pass_and_fail_qcprot_newton(n_sel, weighted):
    """Each flagged family: its key matrices are degenerate (the data is what
    it claims), pair_lambda is inside the bound, and Newton's iteration alone
    -- the epilogue as it was -- is outside it by 100 x or more."""
    from rmsf_amd import _lib
    for family, a, e0, wt in flagged(n_sel, weighted):
        Z.assert_degenerate(a, family)
        lam, path = pair_lambda(a, e0)
        new = ratios(2.0 * (e0 - lam) / wt, a, e0, wt)
        rmsd, steps = oracle_rmsd(a, e0, wt)
        old = ratios(rmsd * rmsd, a, e0, wt)
        print(f"n_sel={n_sel} weighted={weighted} {family}: Newton steps {steps.min()}..{steps.max()}, "
              f"ratio to the bound: Newton alone {old.max():.3e}, pair_lambda {new.max():.3e}")
        assert new.max() <= 1.0, family
        assert np.all(path != _lib.RMSF_PAIR_NEWTON), family
        assert old.max() >= 100.0, family
