"""Response matrices on the CPU (numpy only): the yardstick of nusi_plan_response_apply, and -- cascade_host,
response_mass_host, compose_host below -- of the mass-resolved response and the source's flavour composition.

Every flux the library returns is linear in the source.  ``Plan.response`` hands out the linear map of a parameter
point, G[n][k][b] = the flux of mass state k in bin b per unit of the source-axis bin integral S[n]
(include/nusi.h), and a spectrum's flux is then one matrix-vector product::

    G, G_fla = plan.response([point])                       # (1, M, 3, N) each, once per parameter point
    lo, hi, z = plan.source_axis()
    S = sources.bin_integrals(sources.exp_cutoff(2.3, 3e15), lo, hi)
    flux_fla = response.apply_host(G_fla[0], S, scale=1e-8)   # (3, N); Plan.apply_response does it on the GPU

``apply_host`` is the sum nusi_plan_response_apply defines, in its order: the terms n = 1 .. M-1 ascending, each
product rounded, then the sum rounded (no fma), then the scale -- so the GPU kernel's output equals it bit for bit.
"""
import numpy as np


def apply_host(G, S, scale=None):
    """out[..., q, :, :] = scale[q] * sum_{n=1}^{M-1} G[..., n, :, :] * S[q, n], summed in ascending n.

    G: (M, 3, N) or (ntab, M, 3, N).  S: (M,) or (Q, M).  scale: None (= 1), a number or (Q,).
    Returns (3, N) for one table and one spectrum vector, with a leading ntab and / or Q axis otherwise."""
    G = np.asarray(G, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    one_tab, one_q = G.ndim == 3, S.ndim == 1
    Gt = G[None] if one_tab else G
    Sq = S[None] if one_q else S
    if Gt.ndim != 4 or Sq.ndim != 2 or Gt.shape[1] != Sq.shape[1]:
        raise ValueError("apply_host: G (.., M, 3, N) and S (.., M) do not match: %s, %s" % (G.shape, S.shape))
    ntab, M = Gt.shape[:2]
    Q = Sq.shape[0]
    acc = np.zeros((ntab, Q) + Gt.shape[2:])
    for n in range(1, M):
        term = Gt[:, None, n] * Sq[None, :, n, None, None]     # rounded products ...
        acc = acc + term                                       # ... then the rounded sum
    if scale is not None:
        sc = np.broadcast_to(np.asarray(scale, dtype=np.float64), (Q,))
        acc = sc[None, :, None, None] * acc
    if one_q:
        acc = acc[:, 0]
    if one_tab:
        acc = acc[0]
    return acc


# ---------------------------------------------------------------------------
# The cascade itself on the host, and the mass-resolved response (include/nusi.h "Mass-resolved response matrices")
# ---------------------------------------------------------------------------
def tabulated_src_host(step_c, norm, w, z, S, N):
    """The tabulated source term of every (step i, bin b), shape (Nz, N): step_c[i] * ((norm / 3.0) * (w[i] / (1 + z[i]))
    * S[b + i]) -- tabulated_src of the kernels, the same operations (row 0 is zero: no source at step 0)."""
    step_c, w, z, S = (np.asarray(a, dtype=np.float64) for a in (step_c, w, z, S))
    Nz = step_c.size
    out = np.zeros((Nz, N))
    for i in range(1, Nz):
        out[i] = step_c[i] * ((norm / 3.0) * (w[i] / (1 + z[i])) * S[i:i + N])
    return out


def _lu3(A):
    """gsl_linalg_LU_decomp on 3x3 (partial pivoting, Doolittle), lu3_factor of the kernels, elementwise over the
    leading axes.  A: list of lists of arrays, changed in place; returns the permutation as three integer arrays."""
    shape = A[0][0].shape
    perm = [np.full(shape, k, dtype=np.int64) for k in range(3)]
    for j in range(2):
        amax = np.abs(A[j][j])
        ip = np.full(shape, j, dtype=np.int64)
        for i in range(j + 1, 3):
            c = np.abs(A[i][j]) > amax
            amax = np.where(c, np.abs(A[i][j]), amax)
            ip = np.where(c, i, ip)
        for i in range(j + 1, 3):
            sw = ip == i
            if sw.any():
                for c in range(3):
                    A[j][c], A[i][c] = np.where(sw, A[i][c], A[j][c]), np.where(sw, A[j][c], A[i][c])
                perm[j], perm[i] = np.where(sw, perm[i], perm[j]), np.where(sw, perm[j], perm[i])
        ajj = A[j][j]
        nz = ajj != 0.0
        den = np.where(nz, ajj, 1.0)
        for i in range(j + 1, 3):
            aij = A[i][j] / den
            for c in range(j + 1, 3):
                A[i][c] = np.where(nz, A[i][c] - aij * A[j][c], A[i][c])
            A[i][j] = np.where(nz, aij, A[i][j])
    return perm


def cascade_host(Gam, aT, al_packed, Emin, Emax, step_c, step_s, u, U2, non_resonant, src):
    """The implicit redshift cascade and its finalise (nuSIprop.hpp:255-336) with the source term per mass state, on
    the host: the scalar kernel k_cascade's loop nest operation for operation -- the records (Zdr, M = I + offdiag, its
    LU with GSL's pivot rule), the push of each solved bin into the bins below (non-resonant) or the resonant-only
    running sum, the 3x3 solve, the finalise -- every product, quotient and sum rounded separately in the kernel's
    order.

    Gam, aT (..., T) and al_packed (..., T (T - 1) / 2): a point's Stage-A tables (Plan.tables); Emin, Emax (N,): the
    energy bins' edges (Plan.source_axis()[0][:N], [1][:N]); step_c, step_s (Nz,): Plan.step_constants(); u (..., 3):
    the couplings' |U_flav,k|^2; U2 (3, 3) or (9,): the finalise's |U|^2; non_resonant: bool;
    src (..., 3, Nz, N): the source term of (mass state k, step i, bin b), step_c included (tabulated_src_host).
    Vectorised over the leading axes only (the tables' leading axes broadcast against the source's).
    Returns (flux, flux_fla) of shape (..., 3, N)."""
    Gam, aT, Al, Emin, Emax, step_c, step_s, u, src = (np.asarray(a, dtype=np.float64) for a in
                                                       (Gam, aT, al_packed, Emin, Emax, step_c, step_s, u, src))
    U2 = np.asarray(U2, dtype=np.float64).reshape(3, 3)
    N, Nz = Emin.size, step_c.size
    if src.shape[-3:] != (3, Nz, N):
        raise ValueError("cascade_host: src must have shape (..., 3, %d, %d), got %s" % (Nz, N, src.shape))
    L = np.broadcast_shapes(src.shape[:-3], Gam.shape[:-1], u.shape[:-1])
    nonres = bool(non_resonant)
    uk = [u[..., k] for k in range(3)]
    ukb = [x[..., None] for x in uk]
    dE = Emax - Emin
    F = [np.zeros(L + (N,)) for _ in range(3)]
    bidx = np.arange(N)
    for i in range(Nz - 1, 0, -1):
        c, s = step_c[i], step_s[i]
        # the flux-independent quantities of every bin of the step (elementwise over bins, as the kernel's lanes)
        Gw, Aw = s * Gam[..., bidx + i - 1], s * aT[..., bidx + i - 1]
        Zd = [1.0 + c * (Gw * ukb[k] - Aw * (ukb[k] * ukb[k])) / dE for k in range(3)]
        M = [[np.ones_like(Zd[0]) if k == l else (Aw * ukb[k] * ukb[l] / dE) / Zd[k] for l in range(3)] for k in range(3)]
        pm = _lu3(M)
        rz = [1.0 / Zd[k] for k in range(3)]
        ru = [1.0 / M[k][k] for k in range(3)]
        sde = np.broadcast_to(s / dE if nonres else dE, Zd[0].shape)
        acc = np.zeros(L + (N,))
        next_acc, racc = np.zeros(L), np.zeros(L)
        px = [np.zeros(L) for _ in range(3)]
        for b in range(N - 1, -1, -1):
            accb = acc[..., b - 1].copy() if b > 0 else 0.0   # (before this bin's pushes)
            if nonres:
                add = c * next_acc
            else:
                if b != N - 1:
                    Sres = uk[0] * px[0] + uk[1] * px[1] + uk[2] * px[2]
                    rd = (b + i) * (b + i - 1) // 2 + (b + i - 1)
                    racc = racc + Sres * (s * Al[..., rd]) / (Emax[b + 1] - Emin[b + 1]) / sde[..., b]
                add = c * racc * sde[..., b]
            v = [(F[k][..., b] + (src[..., k, i, b] + uk[k] * add)) * rz[k][..., b] for k in range(3)]
            x = [np.where(pm[k][..., b] == 0, v[0], np.where(pm[k][..., b] == 1, v[1], v[2])) for k in range(3)]
            x[1] = x[1] - M[1][0][..., b] * x[0]
            x[2] = x[2] - M[2][0][..., b] * x[0]
            x[2] = x[2] - M[2][1][..., b] * x[1]
            x[2] = x[2] * ru[2][..., b]
            x[1] = (x[1] - M[1][2][..., b] * x[2]) * ru[1][..., b]
            x[0] = (x[0] - M[0][1][..., b] * x[1] - M[0][2][..., b] * x[2]) * ru[0][..., b]
            for k in range(3):
                F[k][..., b] = x[k]
            px = x
            if nonres and b > 0:
                Tb = (uk[0] * x[0] + uk[1] * x[1] + uk[2] * x[2]) * sde[..., b]
                r = b + i - 1
                base = r * (r - 1) // 2 + (i - 1)
                next_acc = accb + Al[..., base + b - 1] * Tb
                if b - 1 > 0:
                    acc[..., :b - 1] += Al[..., base:base + b - 1] * np.asarray(Tb)[..., None]
    f = [F[k] / dE for k in range(3)]
    flux = np.stack(f, axis=-2)
    fla = np.stack([U2[q, 0] * f[0] + U2[q, 1] * f[1] + U2[q, 2] * f[2] for q in range(3)], axis=-2)
    return flux, fla


def impulse_sources(step_c, w, z, N):
    """The source terms of the mass-resolved response's columns, shape (3, M, 3, Nz, N): column (j, n) has
    delta_{k j} * [b + i == n] * sig3[i] at (k, i, b), sig3[i] = step_c[i] * (w[i] / (1 + z[i])) for i >= 1."""
    step_c, w, z = (np.asarray(a, dtype=np.float64) for a in (step_c, w, z))
    Nz = step_c.size
    M = N + Nz - 1
    src = np.zeros((3, M, 3, Nz, N))
    for i in range(1, Nz):
        sig3 = step_c[i] * (w[i] / (1 + z[i]))
        for b in range(N):
            for j in range(3):
                src[j, b + i, j, i, b] = sig3
    return src


def response_mass_host(Gam, aT, al_packed, Emin, Emax, step_c, step_s, z, w, u, U2, non_resonant):
    """The mass-resolved response matrices (G3, G3_fla) of one table, shape (3, M, 3, N), by the definition of
    include/nusi.h: cascade_host on the impulse sources (impulse_sources) of the redshift weights w [Nz]."""
    return cascade_host(Gam, aT, al_packed, Emin, Emax, step_c, step_s, u, U2, non_resonant,
                        impulse_sources(step_c, w, z, np.asarray(Emin).size))


def compose_host(A3, kappa):
    """out[t, c] = (kappa[t, c, 0] * A3[t, 0] + kappa[t, c, 1] * A3[t, 1]) + kappa[t, c, 2] * A3[t, 2], each product and
    sum rounded (nusi_plan_response_compose's expression, so Plan.compose_response equals it bit for bit).

    A3: (ntab, 3, ...) -- G3 / G3_fla of Plan.response_mass, or folded rows (ntab, 3, M, C).  kappa: (3,), (Qc, 3) or
    (ntab, Qc, 3), finite and >= 0 (sources.mass_fractions).  Returns (ntab, ...) for a kappa of shape (3,), else
    (ntab, Qc, ...)."""
    A = np.asarray(A3, dtype=np.float64)
    k = np.asarray(kappa, dtype=np.float64)
    if A.ndim < 3 or A.shape[1] != 3:
        raise ValueError("compose_host: A3 must have shape (ntab, 3, ...), got %s" % (A.shape,))
    if k.ndim == 0 or k.ndim > 3 or k.shape[-1] != 3 or (k.ndim == 3 and k.shape[0] != A.shape[0]):
        raise ValueError("compose_host: kappa must have shape (3,), (Qc, 3) or (ntab, Qc, 3), got %s" % (k.shape,))
    if not (np.isfinite(k).all() and (k >= 0).all()):
        raise ValueError("compose_host: a mass fraction is negative or not finite")
    one = k.ndim == 1
    kb = np.broadcast_to(k[None] if one else k, (A.shape[0],) + (k.shape[-2:] if not one else (1, 3)))
    kx = kb.reshape(kb.shape + (1,) * (A.ndim - 2))          # (ntab, Qc, 3, 1, ...)
    out = (kx[:, :, 0] * A[:, None, 0] + kx[:, :, 1] * A[:, None, 1]) + kx[:, :, 2] * A[:, None, 2]
    return out[:, 0] if one else out
