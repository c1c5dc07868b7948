"""High-precision host reference of the per-frame transform record (R, COM,
rmsd) that ``rmsf_superpose*`` writes -- TEST INFRASTRUCTURE ONLY.

Independent of the QCP restatement in ``rmsf_oracle``: the rotation is the
quaternion of the top eigenvector of the 4x4 key matrix K(A) (Horn 1987 /
Theobald 2005), taken from a batched ``np.linalg.eigh``; R is quadratic in
the quaternion, so the eigenvector's sign does not matter.  Everything is
vectorised over frames and computed relative to the frame's first selected
atom, so coordinates far from the origin cost no precision.

As RMSF.py:94-97 / 43-51 do: the frame is centred on its (mass-weighted)
centre of mass, and the inner product A and the inner sums G are unweighted.
"""
from __future__ import annotations

import numpy as np

from . import rmsf_oracle as O

# the constants of stats_plan() (csrc/rmsf_kernels.hip), restated
TILE_ATOMS = 32
GROUP_FRAMES = 64
ROUND_GROUPS = 768
MAX_GROUPS = 3072
ROUND_UNITS = 768 * 160
PARTIAL_BYTES = 16 * 64 * 8  # one (segment) partial: 16 sums x 64 frames of f64


def stats_plan(n_sel: int, n_frames: int) -> dict:
    """stats_plan() of csrc/rmsf_kernels.hip restated: the balanced grid of
    k_frame_stats.  ``ranges[b]`` = the units [lo, hi) of workgroup b (unit =
    group * ntiles + tile); ``segments[b]`` = its (group, first tile, one past
    the last tile) runs, in order."""
    ntiles = -(-n_sel // TILE_ATOMS)
    ngroups = max(1, -(-n_frames // GROUP_FRAMES))
    T = ntiles * ngroups
    rounds = min(MAX_GROUPS // ROUND_GROUPS, max(1, (T + ROUND_UNITS // 2) // ROUND_UNITS))
    G = max(1, min(ROUND_GROUPS * rounds, T))
    length = -(-T // G)
    P = -(-length // ntiles) + 1
    ranges = [(T * b // G, T * (b + 1) // G) for b in range(G)]
    segments = []
    for lo, hi in ranges:
        segs = []
        while lo < hi:
            g = lo // ntiles
            t_lo = lo - g * ntiles
            t_hi = min(ntiles, t_lo + (hi - lo))
            segs.append((g, t_lo, t_hi))
            lo += t_hi - t_lo
        segments.append(segs)
    return dict(ntiles=ntiles, ngroups=ngroups, T=T, G=G, len=length, P=P, ranges=ranges, segments=segments)


def key_matrix(A: np.ndarray) -> np.ndarray:
    """K(A) [..., 4, 4] of the inner product A [..., 9] (row-major,
    A[3a + b] = sum mob_a ref_b): its top eigenvector is the quaternion of
    the rotation R with mob @ R ~ ref."""
    A = np.asarray(A, dtype=np.float64)
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (A[..., i] for i in range(9))
    K = np.empty(A.shape[:-1] + (4, 4))
    K[..., 0, 0] = Sxx + Syy + Szz
    K[..., 1, 1] = Sxx - Syy - Szz
    K[..., 2, 2] = -Sxx + Syy - Szz
    K[..., 3, 3] = -Sxx - Syy + Szz
    K[..., 0, 1] = K[..., 1, 0] = Syz - Szy
    K[..., 0, 2] = K[..., 2, 0] = Szx - Sxz
    K[..., 0, 3] = K[..., 3, 0] = Sxy - Syx
    K[..., 1, 2] = K[..., 2, 1] = Sxy + Syx
    K[..., 1, 3] = K[..., 3, 1] = Szx + Sxz
    K[..., 2, 3] = K[..., 3, 2] = Syz + Szy
    return K


def quaternion_rotation(q: np.ndarray) -> np.ndarray:
    """R [..., 3, 3] (applied as x @ R) of unit quaternions q [..., 4]."""
    q1, q2, q3, q4 = (q[..., i] for i in range(4))
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = q1 * q1 + q2 * q2 - q3 * q3 - q4 * q4
    R[..., 0, 1] = 2 * (q2 * q3 + q1 * q4)
    R[..., 0, 2] = 2 * (q4 * q2 - q1 * q3)
    R[..., 1, 0] = 2 * (q2 * q3 - q1 * q4)
    R[..., 1, 1] = q1 * q1 - q2 * q2 + q3 * q3 - q4 * q4
    R[..., 1, 2] = 2 * (q3 * q4 + q1 * q2)
    R[..., 2, 0] = 2 * (q4 * q2 + q1 * q3)
    R[..., 2, 1] = 2 * (q3 * q4 - q1 * q2)
    R[..., 2, 2] = q1 * q1 - q2 * q2 - q3 * q3 + q4 * q4
    return R


def top_eigen(A: np.ndarray):
    """(lambda [...], R [..., 3, 3]): the top eigenvalue of K(A) and the
    rotation of its eigenvector."""
    w, v = np.linalg.eigh(key_matrix(A))
    return w[..., -1], quaternion_rotation(v[..., :, -1])


def _centre(x: np.ndarray, masses):
    """(pivot + c, x - pivot - c): the (mass-weighted) centre of mass and the
    centred coordinates of x [..., N, 3], both through sums relative to the
    first atom."""
    p = x[..., :1, :]
    xp = x - p
    if masses is None:
        c = xp.sum(axis=-2) / x.shape[-2]
    else:
        m = np.asarray(masses, dtype=np.float64)
        c = (xp * m[:, None]).sum(axis=-2) / m.sum()
    return p[..., 0, :] + c, xp - c[..., None, :]


def records(frames: np.ndarray, reference: np.ndarray, masses=None) -> dict:
    """The transform records of ``frames`` (float32 [F, N, 3], the selected
    atoms in selection order) superposed on ``reference`` (float32 [N, 3]):
    com [F, 3], R [F, 3, 3], rmsd [F], and the intermediates A [F, 9], E0,
    lam, g_ref, g_mob."""
    x = np.asarray(frames).astype(np.float64)
    n = x.shape[1]
    com, y = _centre(x, masses)
    _, r = _centre(np.asarray(reference).astype(np.float64), masses)
    A = np.einsum("fia,ib->fab", y, r).reshape(-1, 9)
    g_mob = np.einsum("fia,fia->f", y, y)
    g_ref = float(np.einsum("ia,ia->", r, r))
    E0 = 0.5 * (g_mob + g_ref)
    lam, R = top_eigen(A)
    rmsd = np.sqrt(np.abs(2.0 * (E0 - lam) / n))
    return dict(com=com, R=R, rmsd=rmsd, A=A, E0=E0, lam=lam, g_ref=g_ref, g_mob=g_mob)


def sample_frames(n_frames: int, most: int = 200) -> np.ndarray:
    """The first and last frame of every 64-frame group and frames 0, 63, 64
    and n_frames - 1; evenly thinned to ``most`` frames, keeping both ends."""
    g = np.arange(0, n_frames, GROUP_FRAMES)
    f = np.unique(np.clip(np.concatenate([g, g + GROUP_FRAMES - 1, [0, 63, 64, n_frames - 1]]), 0, n_frames - 1))
    if len(f) > most:
        f = f[np.unique(np.round(np.linspace(0, len(f) - 1, most)).astype(np.int64))]
    return f


def oracle_rotations(frames: np.ndarray, reference: np.ndarray, masses, which) -> np.ndarray:
    """RMSF.py:94-97 + get_rotation_matrix (the QCP restatement of
    ``rmsf_oracle``) for the frames ``which``: R [len(which), 3, 3]."""
    _, ref_c = O.centred_reference(np.asarray(reference), masses)
    out = np.empty((len(which), 3, 3))
    for k, f in enumerate(which):
        p = np.asarray(frames[f])
        com = O.center_of_mass(p, masses)
        out[k] = O.get_rotation_matrix(ref_c, p.astype(np.float64) - com, p.shape[0])
    return out


def qcp_column_norms2(A, lam: float) -> np.ndarray:
    """The squared norms of the four candidate quaternions of qcprot's
    FastCalcRMSDAndRotation: the rows of the adjugate of K(A) - lam I, in the
    order the solver tries them (it takes the first that reaches 1e-6 and
    returns the identity if none does)."""
    M = key_matrix(np.asarray(A, dtype=np.float64)) - lam * np.eye(4)
    cof = np.empty((4, 4))
    for i in range(4):
        for j in range(4):
            minor = np.delete(np.delete(M, i, axis=0), j, axis=1)
            cof[i, j] = (-1) ** (i + j) * np.linalg.det(minor)
    return (cof * cof).sum(axis=1)


def qcp_exit(A, evecprec: float = 1e-6):
    """(exit, norms2): which candidate (1-4) the solver takes for the inner
    product A, 0 for the identity exit, with lam the top eigenvalue of K(A)."""
    lam = float(np.linalg.eigvalsh(key_matrix(np.asarray(A, dtype=np.float64)))[-1])
    n2 = qcp_column_norms2(A, lam)
    for k in range(4):
        if n2[k] >= evecprec:
            return k + 1, n2
    return 0, n2
