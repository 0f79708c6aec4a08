"""Folding fluxes with a detector on the CPU (numpy only): the yardstick of the plan's detector calls and the user's
host path.

A fit compares binned event counts, not fluxes.  The detector of a plan is one matrix, D[c][f][b] = the expected
number of events in reconstructed-energy bin c per unit of flux_fla[f][b] (include/nusi.h), and the reduction is linear,
so it commutes with the response apply: D . (G_fla . S) = (D . G_fla) . S.  Folding a response matrix once gives
R[n][c], M x C doubles, and every spectrum is then a C-vector of expected counts::

    D = detector.matrix(lo[:N], hi[:N], aeff, migration, exposure)       # (C, 3, N)
    plan.set_detector(D, background=b)
    R = plan.fold_response(G_fla)                                       # (ntab, M, C); fold_host on the CPU
    mu, nll = plan.events(R, spectra, scale=1e-8, data=counts)          # events_host + poisson_host on the CPU
    ahat, nll_hat, _, st = plan.profile(R, spectra, data=counts)        # profile_host on the CPU: min over the scale

``fold_host`` has no defined summation order (neither has the GPU's, which runs on the matrix cores): with every term
non-negative, either is within gamma_K = K u / (1 - K u), K = 3 N, u = 2^-53, of the exact sum.  ``events_host`` and
``poisson_host`` are the sums nusi_plan_response_events defines, in its order, so mu agrees bit for bit and nll to the
last bits of the log.  ``profile_host`` is the iteration nusi_plan_response_profile defines, operation for operation
(``tree`` is its sum over the bins), so ahat, mu and the status word agree bit for bit as well.  ``fit_host`` is the
same for nusi_plan_response_fit, the fit that floats K background templates with the signal::

    plan.set_templates(T, prior=(mean, sigma))                           # (K, C), K <= FIT_TEMPLATES_MAX
    theta, nll, mu, st = plan.fit(R, spectra, data=counts)              # fit_host on the CPU: theta (ntab, Q, 1 + K)

``fit_components_host`` is nusi_plan_response_fit_components, that fit with J = 2 .. 3 signal components per table and
spectrum -- a stack R3 (ntab, J, M, C), e.g. the folded mass-resolved rows composed onto the pure flavours -- whose shares
``composition`` reads off, and ``composition_statistic`` the statistic of a held composition against that free fit::

    theta, nll, mu, st = plan.fit_components(R3, spectra, data=counts)  # fit_components_host: theta (ntab, Q, J + K)
    total, frac = detector.composition(theta, 3)                         # the scale and the fitted shares

``ensemble_host`` loops either over P data sets and keeps, per data set and table, the best spectrum's record under
``argbest``'s key (isnan(nll), nll, q) -- nusi_plan_response_ensemble's selection rule; ``pseudo_data`` draws the toys::

    toys = detector.pseudo_data(mu[0, 0], 1000, np.random.default_rng(1))   # (P, C) Poisson counts
    q, nll, theta, st = plan.ensemble(R, spectra, toys)                  # ensemble_host on the CPU: (P, ntab) records

``fit_fixed_host`` is nusi_plan_response_fit_fixed, the fit with the signal's scale held and only the templates
floating (the background-only fit at scale 0), and ``limit_host`` nusi_plan_response_limit: the best fit and the
scales at which q(a) = 2 (min_theta f(a, theta) - min f) = delta, by Newton's iteration in a with a conditional fit per
step -- both the header's text operation for operation::

    theta0, nll0, mu0, st0 = plan.fit_fixed(R, spectra, 0.0, data=counts)     # fit_fixed_host on the CPU
    lo, hi, theta_hat, nll_hat, st = plan.limit(R, spectra, counts, delta=2.706, which="upper")   # limit_host

``draw_host`` is nusi_plan_draw_counts, the counter-based generator of Poisson counts (``philox4x32``, ``uniforms``,
``loggam`` are its parts), every integer the GPU's with the same exp and log, and ``inject_host`` nusi_plan_response_inject:
per table and spectrum the statistic q(a_test) on toys drawn from a_inj s + sum_j theta_inj_j T_j + B, a loop of the forms
above over draw_host's toys::

    toys = plan.draw(mu0[0, 0], 1000, seed=7)                                 # draw_host on the CPU
    band_theta, band_q, tally, exceed = plan.inject(R, spectra, hi[0], 1000, seed=7, mode="upper", q_obs=2.706)   # inject_host
"""
import numpy as np

BINS_MAX = 64       # NUSI_DETECTOR_BINS_MAX
# the profile's status word (include/nusi.h NUSI_FIT_*): the step count in the low 8 bits, flags above
FIT_ITER_MAX = 64
FIT_STEPS_MASK = 0xFF
FIT_FLAT, FIT_BOUNDARY, FIT_NOT_CONVERGED, FIT_INFINITE = 0x100, 0x200, 0x400, 0x800
# the fit with floating templates (nusi_plan_response_fit) adds: a singular Newton system, one bit per component that ends
# at zero (FIT_ZERO << j) and the halvings of all its steps (saturating at FIT_TRIALS_MASK) from bit FIT_TRIALS_SHIFT
FIT_TEMPLATES_MAX = 3
FIT_SIGNALS_MAX = 3  # the signal components of fit_components_host (NUSI_FIT_SIGNALS_MAX)
FIT_TRIALS_MAX = 64
FIT_SINGULAR = 0x1000
FIT_ZERO = 0x10000
FIT_TRIALS_SHIFT, FIT_TRIALS_MASK = 24, 0x7F
# the limits on the signal's scale (nusi_plan_response_limit): the sides asked for, the outer cap, and a side's status word:
# the outer steps in the low 8 bits (LIMIT_STEPS_MASK), the flags, the inner Newton steps (saturating) from LIMIT_INNER_SHIFT
LIMIT_LOWER, LIMIT_UPPER = 1, 2
LIMIT_ITER_MAX = 64
LIMIT_STEPS_MASK = 0xFF
LIMIT_AT_ZERO, LIMIT_UNBOUNDED, LIMIT_NO_FIT, LIMIT_NOT_CONVERGED = 0x100, 0x200, 0x400, 0x800
LIMIT_INNER_SHIFT, LIMIT_INNER_MASK = 16, 0x7FFF


def gamma(K):
    """gamma_K = K u / (1 - K u), u = 2^-53: the relative error bound of a sum of K non-negative products."""
    u = 2.0 ** -53
    return K * u / (1.0 - K * u)


def _ceil_log2(C):
    L = 0
    while (1 << L) < C:
        L += 1
    return L


def _squeeze(one_tab, one_q, *arrays):
    """The arrays (ntab, Q, ..) without the axes that a single table (R of two axes) or spectrum (S of one) added."""
    if one_q:
        arrays = [a[:, 0] for a in arrays]
    if one_tab:
        arrays = [a[0] for a in arrays]
    return tuple(arrays)


def fold_host(rows, D):
    """out[..., c] = sum_{f, b} rows[..., f, b] * D[c, f, b].  rows: (..., 3, N) -- flux_fla (n, 3, N) or G_fla
    (ntab, M, 3, N); D: (C, 3, N).  No background, no defined order (a matrix product)."""
    rows = np.asarray(rows, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 3 or rows.ndim < 2 or rows.shape[-2:] != D.shape[1:]:
        raise ValueError("fold_host: rows (.., 3, N) and D (C, 3, N) do not match: %s, %s" % (rows.shape, D.shape))
    K = D.shape[1] * D.shape[2]
    out = rows.reshape(-1, K) @ D.reshape(D.shape[0], K).T
    return out.reshape(rows.shape[:-2] + (D.shape[0],))


def events_host(R, S, scale=None, background=None):
    """mu[..., q, c] = scale[q] * acc + background[c], acc = sum_{n=1}^{M-1} R[..., n, c] * S[q, n] in ascending n
    (each product rounded, then the sum: response.apply_host's loop).

    R: (M, C) or (ntab, M, C).  S: (M,) or (Q, M).  scale: None (= 1), a number or (Q,).  background: None (= 0),
    a number or (C,)."""
    R = np.asarray(R, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    one_tab, one_q = R.ndim == 2, S.ndim == 1
    Rt = R[None] if one_tab else R
    Sq = S[None] if one_q else S
    if Rt.ndim != 3 or Sq.ndim != 2 or Rt.shape[1] != Sq.shape[1]:
        raise ValueError("events_host: R (.., M, C) and S (.., M) do not match: %s, %s" % (R.shape, S.shape))
    ntab, M, C = Rt.shape
    Q = Sq.shape[0]
    acc = np.zeros((ntab, Q, C))
    for n in range(1, M):
        term = Rt[:, None, n] * Sq[None, :, n, None]      # rounded products ...
        acc = acc + term                                  # ... then the rounded sum
    sc = np.ones(Q) if scale is None else np.broadcast_to(np.asarray(scale, dtype=np.float64), (Q,))
    bg = np.zeros(C) if background is None else np.broadcast_to(np.asarray(background, dtype=np.float64), (C,))
    mu = sc[None, :, None] * acc                          # two roundings: the scale ...
    mu = mu + bg[None, None, :]                           # ... and the background
    return _squeeze(one_tab, one_q, mu)[0]


def poisson_host(mu, data, log=np.log):
    """nll[...] = sum over c ascending, from 0.0, of mu_c - data_c * log(mu_c) -- mu_c where data_c == 0 (the log is
    not evaluated) -- each operation rounded: the Poisson negative log-likelihood without its data-only constant.
    +inf where data_c > 0 and mu_c == 0.  mu: (..., C); data: (C,); log: a scalar function of a float."""
    mu = np.asarray(mu, dtype=np.float64)
    data = np.asarray(data, dtype=np.float64)
    if data.ndim != 1 or mu.ndim < 1 or mu.shape[-1] != data.shape[0]:
        raise ValueError("poisson_host: mu (.., C) and data (C,) do not match: %s, %s" % (mu.shape, data.shape))
    flat = mu.reshape(-1, data.shape[0])
    out = np.zeros(flat.shape[0])
    for i in range(flat.shape[0]):
        s = 0.0
        for c in range(data.shape[0]):
            m, d = float(flat[i, c]), float(data[c])
            if d == 0.0:
                term = m
            elif m == 0.0:
                term = float("inf")
            else:
                term = m - d * float(log(m))
            s = s + term
        out[i] = s
    return out.reshape(mu.shape[:-1])


def tree(x):
    """The pairwise sum over the last axis that a butterfly over neighbouring lanes computes: pad to P = 2^ceil(log2 C)
    entries with +0.0, then replace the vector by the sums of adjacent pairs (0+1, 2+3, ..) until one value is left."""
    x = np.asarray(x, dtype=np.float64)
    C = x.shape[-1]
    v = np.zeros(x.shape[:-1] + (1 << _ceil_log2(C),))
    v[..., :C] = x
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _signal(who, R, S, data):
    """The front of profile_host and fit_host: (s (ntab, Q, C) = events_host's accumulator, the checked data (C,),
    one_tab, one_q)."""
    R = np.asarray(R, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    data = np.asarray(data, dtype=np.float64)
    one_tab, one_q = R.ndim == 2, S.ndim == 1
    s = events_host(R[None] if one_tab else R, S[None] if one_q else S)           # 1.0 * acc + 0.0: acc itself
    C = s.shape[-1]
    if data.shape != (C,):
        raise ValueError("%s: data must have shape (%d,), got %s" % (who, C, data.shape))
    if not np.all(np.isfinite(data)) or np.any(data < 0):
        raise ValueError("%s: a datum is negative or not finite" % who)
    return s, data, one_tab, one_q


def profile_host(R, S, data, background=None, log=np.log):
    """The Poisson statistic profiled over the flux normalisation: for every table and spectrum the a >= 0 that
    minimises -ln L(a s + B | data), s_c = sum_n R[..., n, c] S[q, n] (events_host's accumulator), by the iteration
    nusi_plan_response_profile defines (include/nusi.h) -- the same operations in the same order, so ahat, mu and
    status agree with the GPU bit for bit and nll to the last bits of the log.

    R: (M, C) or (ntab, M, C).  S: (M,) or (Q, M).  data: (C,).  background: None (= 0), a number or (C,).
    Returns (ahat, nll, mu, status): ahat, nll and status (int32: the step count in the low 8 bits, FIT_* flags above)
    of shape (ntab, Q), mu = ahat s + B of shape (ntab, Q, C); the squeezed axes of events_host are squeezed here."""
    s, data, one_tab, one_q = _signal("profile_host", R, S, data)
    C = s.shape[-1]
    B = np.zeros(C) if background is None else np.broadcast_to(np.asarray(background, dtype=np.float64), (C,))
    d = np.broadcast_to(data, s.shape)
    act = (d > 0) & (s > 0)
    S1 = tree(s)
    flat = (S1 == 0) | ~act.any(axis=-1)
    flags = np.where(flat, FIT_FLAT, 0).astype(np.int32)
    steps = np.zeros(S1.shape, dtype=np.int32)
    with np.errstate(all="ignore"):
        x = np.where(act, d / S1[..., None] - B / s, 0.0)
        a = np.where(flat, 0.0, np.maximum(0.0, x.max(axis=-1)))
        run = ~flat
        for it in range(FIT_ITER_MAX):
            if not run.any():
                break
            den = a[..., None] * s                         # two roundings
            den = den + B
            u = np.where(act, s / den, 0.0)                # inactive bins: exactly 0.0 in both sums, never divided
            r = d * u
            h = r * u
            S2, S3 = tree(r), tree(h)
            steps[run] += 1
            g = S1 - S2
            stop = run & ~(g < 0)
            flags[stop & (a == 0)] |= FIT_BOUNDARY
            run = run & ~stop
            an = a + (S2 - S1) / S3
            run = run & (an > a)
            a = np.where(run, an, a)
        flags[run] |= FIT_NOT_CONVERGED
    mu = a[..., None] * s
    mu = mu + B
    flags[np.any((d > 0) & (mu == 0), axis=-1)] |= FIT_INFINITE
    nll = poisson_host(mu, data, log=log)
    return _squeeze(one_tab, one_q, a, nll, mu, steps | flags)


def fit_kappa(C, K, J=1):
    """kappa(C, K) = 2 (ceil(log2 C) + K) + 18: the stop of nusi_plan_response_fit, |g_j| <= kappa u scale_j on the
    computed gradient (include/nusi.h; derived in DESIGN.md sec. 4, "The fit with floating templates").  With J signal
    components (fit_components_host) den has J - 1 more products: K -> J - 1 + K."""
    return 2 * (_ceil_log2(C) + J - 1 + K) + 18


def K_fit(C, K, J=1):
    """The bound on the EXACT residual of a converged fit, in units of u scale_j: the stop's kappa plus the rounding of
    the computed gradient, ceil(log2 C) + 2 K + 8, plus one for the computed scale (K -> J - 1 + K with J signal
    components: 3 ceil(log2 C) + 4 (J - 1 + K) + 27)."""
    return fit_kappa(C, K, J) + _ceil_log2(C) + 2 * (J - 1 + K) + 9


def _prior(K, prior):
    """(mean [1 + K], weight [1 + K]) with the signal's zeros in front: w_j = 1 / (sigma_j sigma_j), 0 = no prior."""
    m, w = np.zeros(1 + K), np.zeros(1 + K)
    if prior is not None:
        mean, sigma = prior
        sigma = np.broadcast_to(np.asarray(np.inf if sigma is None else sigma, dtype=np.float64), (K,))
        mean = np.broadcast_to(np.asarray(0.0 if mean is None else mean, dtype=np.float64), (K,))
        if np.any(np.isnan(sigma)) or np.any(sigma <= 0) or not np.all(np.isfinite(mean)) or np.any(mean < 0):
            raise ValueError("fit: a prior needs a finite mean >= 0 and a width > 0")
        with np.errstate(all="ignore"):
            w[1:] = 1.0 / (sigma * sigma)
        m[1:] = np.where(w[1:] > 0, mean, 0.0)
    return m, w


def _templates(templates, C):
    T = np.asarray(templates, dtype=np.float64)
    if T.ndim == 1:
        T = T[None]
    if T.ndim != 2 or T.shape[1] != C or not 1 <= T.shape[0] <= FIT_TEMPLATES_MAX:
        raise ValueError("fit: templates must have shape (K, %d), K = 1 .. %d, got %s" % (C, FIT_TEMPLATES_MAX, T.shape))
    if not np.all(np.isfinite(T)) or np.any(T < 0) or np.any(T.max(axis=1) == 0):
        raise ValueError("fit: a template entry is negative or not finite, or a template is all zeros")
    return T


def _fit_solve(A, g, fs, n):
    """p = -A^-1 g on the components of the set fs (the others: an identity row and p = 0), by L D L^T in ascending
    order.  Returns (p, singular)."""
    a = [[(A[max(i, j)][min(i, j)] if (fs[i] and fs[j]) else (1.0 if i == j else 0.0)) for j in range(n)] for i in range(n)]
    rhs = [(-g[i] if fs[i] else 0.0) for i in range(n)]
    Lm = [[0.0] * n for _ in range(n)]
    Dg = [0.0] * n
    for i in range(n):
        c = [0.0] * n
        for j in range(i):
            v = a[i][j]
            for k in range(j):
                v = v - c[k] * Lm[j][k]
            c[j] = v
            Lm[i][j] = v / Dg[j]
        dd = a[i][i]
        for k in range(i):
            dd = dd - c[k] * Lm[i][k]
        if not dd > 0.0:
            return None, True
        Dg[i] = dd
    y = [0.0] * n
    for i in range(n):
        v = rhs[i]
        for k in range(i):
            v = v - Lm[i][k] * y[k]
        y[i] = v
    p = [0.0] * n
    for i in range(n - 1, -1, -1):
        v = y[i] / Dg[i]
        for k in range(i + 1, n):
            v = v - Lm[k][i] * p[k]
        p[i] = v
    return p, False


def _fit_one(X, B, d, m, w, ku, J=1):
    """One fit of nusi_plan_response_fit: X (1 + K, C) the signal and the templates, B, d (C,), m, w (1 + K,) the
    priors' means and weights (0 in front), ku = kappa u.  Returns (theta list, status).  J > 1: the fit of
    nusi_plan_response_fit_components, X (J + K, C) with J signal components in front, each under the signal's liveness
    rule; FIT_FLAT when none of them is live, FIT_BOUNDARY when one is and all end at zero."""
    n, C = X.shape
    S1 = [float(v) for v in tree(X)]
    live = [S1[j] > 0.0 and bool(np.any((d > 0) & (X[j] > 0))) for j in range(J)] + [S1[j] > 0.0 for j in range(J, n)]
    sup = B > 0
    for j in range(n):
        if live[j]:
            sup = sup | (X[j] > 0)
    act = (d > 0) & sup
    D0 = float(tree(np.where(act, d, 0.0)))
    dmin = min(1.0, float(np.min(np.where(act, d, 1.0))))
    nl = float(sum(live))
    m = [float(v) for v in m]
    w = [float(v) for v in w]
    th = [(D0 / (nl * S1[j]) if live[j] else 0.0) for j in range(n)]
    the = list(th)
    XX = [(j, k) for j in range(n) for k in range(j, n)]
    JJ, KK = [j for j, _ in XX], [k for _, k in XX]
    flags, steps, halv = 0, 0, 0
    first, p, t, quad, trials = True, [0.0] * n, 1.0, False, 0
    while True:
        den = the[0] * X[0]
        for j in range(1, n):
            den = den + the[j] * X[j]
        den = den + B
        bad = bool(np.any(act & ~(den > 0)))
        wq = np.where(act, d / den, 0.0)
        r = np.where(act, wq / den, 0.0)
        xr = X * r
        sums = tree(np.concatenate([X * wq, xr[JJ] * X[KK]]))
        S2 = [float(v) for v in sums[:n]]
        g = [(S1[j] - S2[j]) + w[j] * (the[j] - m[j]) for j in range(n)]
        changed = True
        if first:
            if bad:
                flags |= FIT_NOT_CONVERGED
                break
        else:
            slope = 0.0
            for j in range(n):
                slope = slope + p[j] * g[j]
            if bad or not (quad or not slope > 0.0):
                if trials == FIT_TRIALS_MAX:
                    flags |= FIT_NOT_CONVERGED
                    break
                trials += 1
                halv += 1
                t = t * 0.5
                the = [th[j] + t * p[j] for j in range(n)]
                continue
            changed = any(the[j] != th[j] for j in range(n))
            steps += 1
        th = list(the)
        free = [live[j] and (th[j] > 0.0 or g[j] < 0.0) for j in range(n)]
        if all(abs(g[j]) <= ku * ((S1[j] + S2[j]) + w[j] * (th[j] + m[j])) for j in range(n) if free[j]):
            break
        if (not first and not changed) or steps == FIT_ITER_MAX:
            flags |= FIT_NOT_CONVERGED
            break
        first = False
        A = [[0.0] * n for _ in range(n)]
        for i, (j, k) in enumerate(XX):
            A[k][j] = float(sums[n + i]) + (w[j] if j == k else 0.0)
        fs = list(free)
        while True:
            p, sing = _fit_solve(A, g, fs, n)
            if sing:
                break
            rm = [fs[j] and th[j] == 0.0 and p[j] < 0.0 for j in range(n)]
            if not any(rm):
                break
            fs = [fs[j] and not rm[j] for j in range(n)]
        acc = 0.0
        if not sing:
            for j in range(n):
                if fs[j]:
                    acc = acc + g[j] * p[j]
        if sing or not acc < 0.0:
            flags |= FIT_SINGULAR
            break
        ratio = [(th[j] / -p[j] if (fs[j] and p[j] < 0.0) else 1.0) for j in range(n)]
        t = 1.0
        for j in range(n):
            if ratio[j] < t:
                t = ratio[j]
        clipped = t < 1.0
        quad = (not clipped) and -acc <= 0.0625 * dmin
        trials = 0
        the = [(0.0 if (clipped and fs[j] and p[j] < 0.0 and ratio[j] == t) else th[j] + t * p[j]) for j in range(n)]
    if not any(live[:J]):
        flags |= FIT_FLAT
    elif all(th[j] == 0.0 for j in range(J)):
        flags |= FIT_BOUNDARY
    for j in range(n):
        if th[j] == 0.0:
            flags |= FIT_ZERO << j
    return th, steps | flags | (min(halv, FIT_TRIALS_MASK) << FIT_TRIALS_SHIFT)


def fit_host(R, S, data, templates, prior=None, background=None, log=np.log):
    """The Poisson statistic minimised over the signal's scale AND the normalisations of K background templates, by the
    iteration nusi_plan_response_fit defines (include/nusi.h), operation for operation: theta, mu and status agree with
    the GPU bit for bit and nll to the last bits of the log.

        mu_c(theta) = theta_0 s_c + sum_j theta_j T_j[c] + B_c,  theta >= 0
        f(theta)    = sum_c (mu_c - data_c log mu_c) + sum_j w_j (theta_j - m_j)^2 / 2,  w_j = 1 / (sigma_j sigma_j)

    R: (M, C) or (ntab, M, C).  S: (M,) or (Q, M).  data: (C,).  templates: (K, C), K = 1 .. FIT_TEMPLATES_MAX, entries
    >= 0, none all zeros.  prior: None or (mean (K,), sigma (K,)), sigma = inf: no prior on that template.  background:
    the fixed part B, None (= 0), a number or (C,).  Returns (theta (ntab, Q, 1 + K), nll (ntab, Q), mu (ntab, Q, C),
    status (ntab, Q) int32): the Newton steps in the low 8 bits, the FIT_* flags, FIT_ZERO << j for every component
    that ends at zero and the halvings of all steps (saturating) from bit FIT_TRIALS_SHIFT; the axes events_host
    squeezes are squeezed here."""
    s, data, one_tab, one_q = _signal("fit_host", R, S, data)
    ntab, Q, C = s.shape
    T = _templates(templates, C)
    K = T.shape[0]
    m, w = _prior(K, prior)
    B = np.zeros(C) if background is None else np.array(np.broadcast_to(np.asarray(background, dtype=np.float64), (C,)))
    ku = fit_kappa(C, K) * 2.0 ** -53
    theta = np.zeros((ntab, Q, 1 + K))
    status = np.zeros((ntab, Q), dtype=np.int32)
    mu = np.zeros((ntab, Q, C))
    X = np.zeros((1 + K, C))
    X[1:] = T
    with np.errstate(all="ignore"):
        for t in range(ntab):
            for q in range(Q):
                X[0] = s[t, q]
                th, st = _fit_one(X, B, data, m, w, ku)
                theta[t, q], status[t, q] = th, st
                den = th[0] * X[0]
                for j in range(1, 1 + K):
                    den = den + th[j] * X[j]
                mu[t, q] = den + B
    status[np.any((data > 0) & (mu == 0), axis=-1)] |= FIT_INFINITE
    nll = poisson_host(mu, data, log=log)
    for j in range(1, 1 + K):                                  # the penalties, ascending j, each operation rounded
        if w[j] > 0:
            dl = theta[..., j] - m[j]
            nll = nll + ((0.5 * w[j]) * dl) * dl
    return _squeeze(one_tab, one_q, theta, nll, mu, status)


def fit_components_host(R3, S, data, templates=None, prior=None, background=None, log=np.log):
    """The fit with J signal components per table and spectrum, by the iteration nusi_plan_response_fit_components
    defines (include/nusi.h) -- nusi_plan_response_fit's with the liveness rule on every signal component and J - 1 + K
    in kappa -- operation for operation: theta, mu and status agree with the GPU bit for bit and nll to the last bits of
    the log.

        mu_c(theta) = sum_{j<J} theta_j s_jc + sum_i theta_{J+i-1} T_i[c] + B_c,  theta >= 0,
        s_j = events_host(R3[:, j], S)

    R3: (J, M, C) or (ntab, J, M, C), J = 1 .. FIT_SIGNALS_MAX, entries finite and >= 0: folded mass-resolved rows,
    ``compose_response`` output (onto the pure flavours: theta_j >= 0 is then the physical flavour triangle), or any
    stack of folded matrices.  S: (M,) or (Q, M).  data: (C,).  templates: None (K = 0, allowed here) or (K, C).  prior,
    background, log: as for fit_host (the priors are the templates').  Returns (theta (ntab, Q, J + K), nll, mu,
    status), squeezed as fit_host squeezes: FIT_FLAT when no signal component is live (the templates are fitted all the
    same), FIT_BOUNDARY when one is and every signal theta_j ends at 0, FIT_ZERO << j for j < J + K.  With J = 1 and
    K >= 1 it is fit_host to the bit."""
    R3 = np.asarray(R3, dtype=np.float64)
    one_tab = R3.ndim == 3
    Rt = R3[None] if one_tab else R3
    if Rt.ndim != 4 or not 1 <= Rt.shape[1] <= FIT_SIGNALS_MAX:
        raise ValueError("fit_components_host: R3 must have shape (.., J, M, C), J = 1 .. %d, got %s" % (FIT_SIGNALS_MAX, R3.shape))
    if not np.all(np.isfinite(Rt)) or np.any(Rt < 0):
        raise ValueError("fit_components_host: an entry of R3 is negative or not finite")
    J = Rt.shape[1]
    s0, data, _, one_q = _signal("fit_components_host", Rt[:, 0], S, data)
    ntab, Q, C = s0.shape
    Sq = np.asarray(S, dtype=np.float64)
    Sq = Sq[None] if one_q else Sq
    s = [s0] + [events_host(Rt[:, j], Sq) for j in range(1, J)]
    T = np.zeros((0, C)) if templates is None else _templates(templates, C)
    K = T.shape[0]
    m1, w1 = _prior(K, prior)                                  # (the fit's, one zero in front: J - 1 more)
    m, w = np.concatenate([np.zeros(J - 1), m1]), np.concatenate([np.zeros(J - 1), w1])
    B = np.zeros(C) if background is None else np.array(np.broadcast_to(np.asarray(background, dtype=np.float64), (C,)))
    ku = fit_kappa(C, K, J) * 2.0 ** -53
    n = J + K
    theta = np.zeros((ntab, Q, n))
    status = np.zeros((ntab, Q), dtype=np.int32)
    mu = np.zeros((ntab, Q, C))
    X = np.zeros((n, C))
    X[J:] = T
    with np.errstate(all="ignore"):
        for t in range(ntab):
            for q in range(Q):
                for j in range(J):
                    X[j] = s[j][t, q]
                th, st = _fit_one(X, B, data, m, w, ku, J)
                theta[t, q], status[t, q] = th, st
                den = th[0] * X[0]
                for j in range(1, n):
                    den = den + th[j] * X[j]
                mu[t, q] = den + B
    status[np.any((data > 0) & (mu == 0), axis=-1)] |= FIT_INFINITE
    nll = poisson_host(mu, data, log=log)
    for j in range(J, n):                                      # the templates' penalties, ascending, each operation rounded
        if w[j] > 0:
            dl = theta[..., j] - m[j]
            nll = nll + ((0.5 * w[j]) * dl) * dl
    return _squeeze(one_tab, one_q, theta, nll, mu, status)


def composition(theta, J):
    """(total, fractions) of a component fit's theta (..., J + K): the sum of the J signal scales (ascending j) and
    their shares theta_j / total, shape (..., J) -- on rows composed onto the pure flavours, the fitted flavour
    composition.  NaN where the total is 0."""
    th = np.asarray(theta, dtype=np.float64)
    if th.ndim < 1 or not 1 <= J <= th.shape[-1]:
        raise ValueError("composition: theta must have shape (.., J + K) with J = %r signal components in front, got %s" % (J, th.shape))
    total = th[..., 0]
    for j in range(1, J):
        total = total + th[..., j]
    with np.errstate(all="ignore"):
        frac = np.where(total[..., None] > 0, th[..., :J] / total[..., None], np.nan)
    return total, frac


def composition_statistic(mu, theta, mu_hat, theta_hat, data, prior=None, log=np.log):
    """(lam, mag): lambda = f(theta) - f(theta_hat) of a fit at a held composition against the free component fit, formed
    as nusi_plan_response_limit forms it (``_limit_lambda``, vectorised): per bin (mu - mu_hat) - data log(mu / mu_hat)
    over the bins with data_c > 0 and mu_hat_c > 0 (mu - mu_hat on the others), ``tree()``, then the templates'
    penalty differences ascending; mag is the same sum over the terms' magnitudes.  q = 2 lambda.

    mu, mu_hat: (..., C).  theta: (..., 1 + K) of ``fit`` (or ahat[..., None] of ``profile``), theta_hat: (..., J + K) of
    the component fit: the templates are the last K = theta.shape[-1] - 1 entries of both.  prior: the templates'
    (mean, sigma) as for fit_host, None = no penalty.  All leading axes broadcast."""
    mu, muh = np.asarray(mu, dtype=np.float64), np.asarray(mu_hat, dtype=np.float64)
    th, thh = np.asarray(theta, dtype=np.float64), np.asarray(theta_hat, dtype=np.float64)
    d = np.asarray(data, dtype=np.float64)
    K = th.shape[-1] - 1
    if mu.shape[-1] != d.shape[0] or muh.shape[-1] != d.shape[0] or K < 0 or thh.shape[-1] < K + 1:
        raise ValueError("composition_statistic: mu, mu_hat (.., C), theta (.., 1 + K) and theta_hat (.., J + K) do not match")
    m, w = _prior(K, prior)
    mu, muh = np.broadcast_arrays(mu, muh)
    with np.errstate(all="ignore"):
        lact = (d > 0) & (muh > 0)
        dmu = mu - muh
        ratio = np.where(lact, mu / muh, 1.0)
        lr = np.zeros(ratio.shape)
        flat_r, flat_l, flat_a = ratio.reshape(-1), lr.reshape(-1), lact.reshape(-1)
        for i in np.nonzero(flat_a)[0]:
            flat_l[i] = float(log(flat_r[i])) if flat_r[i] > 0.0 else -np.inf
        lr = flat_l.reshape(ratio.shape)
        pl = np.where(lact, d * lr, 0.0)
        term = np.where(lact, dmu - pl, dmu)
        mag = np.where(lact, np.abs(dmu) + np.abs(pl), np.abs(dmu))
        lam, mg = tree(term), tree(mag)
        for j in range(1, 1 + K):
            if w[j] > 0:
                tj, hj = th[..., j], thh[..., thh.shape[-1] - K + j - 1]
                dj = tj - hj
                sj = (tj - m[j]) + (hj - m[j])
                pd = ((0.5 * w[j]) * dj) * sj
                lam = lam + pd
                mg = mg + np.abs(pd)
    return lam, mg


def _fit_fixed_one(a, s, X, B, d, m, w, ku, start=None):
    """One conditional fit of nusi_plan_response_fit_fixed: the signal s (C,) held at the scale a, X (K, C) the
    templates (K = 0: none, a single evaluation), B, d (C,), m, w (K,) the templates' priors, ku = kappa u.  _fit_one's
    text on the components 1 .. K with the header's differences.  start: None = the header's start; a list = the
    limit's warm start (nusi_plan_response_limit: the start of the header if an active den is not > 0 there).  Returns
    (theta_1 .. theta_K as a list, status, S2_0 = tree(s_c w_c) of the last accepted evaluation)."""
    n, C = X.shape
    a = float(a)
    S1 = [float(v) for v in tree(X)]
    live = [S1[j] > 0.0 for j in range(n)]
    sup = B > 0
    if a > 0.0:
        sup = sup | (s > 0)
    for j in range(n):
        if live[j]:
            sup = sup | (X[j] > 0)
    act = (d > 0) & sup
    D0 = float(tree(np.where(act, d, 0.0)))
    dmin = min(1.0, float(np.min(np.where(act, d, 1.0))))
    nl = float(sum(live))
    m = [float(v) for v in m]
    w = [float(v) for v in w]
    cold = [(D0 / (nl * S1[j]) if live[j] else 0.0) for j in range(n)]
    th = list(cold) if start is None else [float(v) for v in start]
    warm = start is not None
    the = list(th)
    XX = [(j, k) for j in range(n) for k in range(j, n)]
    JJ, KK = np.array([j for j, _ in XX], dtype=int), np.array([k for _, k in XX], dtype=int)
    held = a * s
    S20 = 0.0
    flags, steps, halv = 0, 0, 0
    first, p, t, quad, trials = True, [0.0] * n, 1.0, False, 0
    while True:
        den = held
        for j in range(n):
            den = den + the[j] * X[j]
        den = den + B
        bad = bool(np.any(act & ~(den > 0)))
        wq = np.where(act, d / den, 0.0)
        r = np.where(act, wq / den, 0.0)
        xr = X * r
        sums = tree(np.concatenate([X * wq, xr[JJ] * X[KK], (s * wq)[None]]))
        S2 = [float(v) for v in sums[:n]]
        g = [(S1[j] - S2[j]) + w[j] * (the[j] - m[j]) for j in range(n)]
        changed = True
        if first:
            if bad and warm:                        # (the limit's warm start does not hold here: the header's start)
                warm = False
                th = list(cold)
                the = list(cold)
                continue
            if bad:
                flags |= FIT_NOT_CONVERGED
                break
        else:
            slope = 0.0
            for j in range(n):
                slope = slope + p[j] * g[j]
            if bad or not (quad or not slope > 0.0):
                if trials == FIT_TRIALS_MAX:
                    flags |= FIT_NOT_CONVERGED
                    break
                trials += 1
                halv += 1
                t = t * 0.5
                the = [th[j] + t * p[j] for j in range(n)]
                continue
            changed = any(the[j] != th[j] for j in range(n))
            steps += 1
        th = list(the)
        S20 = float(sums[-1])
        free = [live[j] and (th[j] > 0.0 or g[j] < 0.0) for j in range(n)]
        if all(abs(g[j]) <= ku * ((S1[j] + S2[j]) + w[j] * (th[j] + m[j])) for j in range(n) if free[j]):
            break
        if (not first and not changed) or steps == FIT_ITER_MAX:
            flags |= FIT_NOT_CONVERGED
            break
        first = False
        A = [[0.0] * n for _ in range(n)]
        for i, (j, k) in enumerate(XX):
            A[k][j] = float(sums[n + i]) + (w[j] if j == k else 0.0)
        fs = list(free)
        while True:
            p, sing = _fit_solve(A, g, fs, n)
            if sing:
                break
            rm = [fs[j] and th[j] == 0.0 and p[j] < 0.0 for j in range(n)]
            if not any(rm):
                break
            fs = [fs[j] and not rm[j] for j in range(n)]
        acc = 0.0
        if not sing:
            for j in range(n):
                if fs[j]:
                    acc = acc + g[j] * p[j]
        if sing or not acc < 0.0:
            flags |= FIT_SINGULAR
            break
        ratio = [(th[j] / -p[j] if (fs[j] and p[j] < 0.0) else 1.0) for j in range(n)]
        t = 1.0
        for j in range(n):
            if ratio[j] < t:
                t = ratio[j]
        clipped = t < 1.0
        quad = (not clipped) and -acc <= 0.0625 * dmin
        trials = 0
        the = [(0.0 if (clipped and fs[j] and p[j] < 0.0 and ratio[j] == t) else th[j] + t * p[j]) for j in range(n)]
    for j in range(n):
        if th[j] == 0.0:
            flags |= FIT_ZERO << (j + 1)
    return th, steps | flags | (min(halv, FIT_TRIALS_MASK) << FIT_TRIALS_SHIFT), S20


def fit_fixed_host(R, S, scale, data, templates, prior=None, background=None, log=np.log):
    """The conditional fit: fit_host with the signal's scale HELD at ``scale`` and only the K templates floating, by
    the iteration nusi_plan_response_fit_fixed defines (include/nusi.h), operation for operation: theta, mu and status
    agree with the GPU bit for bit and nll to the last bits of the log.  At scale 0 it is the background-only fit.

    R, S, data, templates, prior, background, log: as for fit_host.  scale: a number or (Q,), finite and >= 0.  Returns
    (theta (ntab, Q, 1 + K) with theta[..., 0] = scale, nll (ntab, Q), mu (ntab, Q, C), status (ntab, Q) int32): the
    word of fit_host without FIT_FLAT, FIT_BOUNDARY and FIT_ZERO << 0, which are never set; the axes events_host
    squeezes are squeezed here."""
    s, data, one_tab, one_q = _signal("fit_fixed_host", R, S, data)
    ntab, Q, C = s.shape
    T = _templates(templates, C)
    K = T.shape[0]
    m, w = _prior(K, prior)
    sc = np.array(np.broadcast_to(np.asarray(scale, dtype=np.float64), (Q,)))
    if not np.all(np.isfinite(sc)) or np.any(sc < 0):
        raise ValueError("fit_fixed_host: a scale is negative or not finite")
    B = np.zeros(C) if background is None else np.array(np.broadcast_to(np.asarray(background, dtype=np.float64), (C,)))
    ku = fit_kappa(C, K) * 2.0 ** -53
    theta = np.zeros((ntab, Q, 1 + K))
    status = np.zeros((ntab, Q), dtype=np.int32)
    mu = np.zeros((ntab, Q, C))
    with np.errstate(all="ignore"):
        for t in range(ntab):
            for q in range(Q):
                th, st, _ = _fit_fixed_one(sc[q], s[t, q], T, B, data, m[1:], w[1:], ku)
                theta[t, q, 0], theta[t, q, 1:], status[t, q] = sc[q], th, st
                den = sc[q] * s[t, q]
                for j in range(K):
                    den = den + th[j] * T[j]
                mu[t, q] = den + B
    status[np.any((data > 0) & (mu == 0), axis=-1)] |= FIT_INFINITE
    nll = poisson_host(mu, data, log=log)
    for j in range(1, 1 + K):                                  # the penalties, ascending j, each operation rounded
        if w[j] > 0:
            dl = theta[..., j] - m[j]
            nll = nll + ((0.5 * w[j]) * dl) * dl
    return _squeeze(one_tab, one_q, theta, nll, mu, status)


def limit_kappa(C, K):
    """kappa_lambda(C, K) = 2 (ceil(log2 C) + K) + 14: the outer stop of nusi_plan_response_limit, |lambda - delta / 2|
    <= kappa_lambda u (magnitudes) (include/nusi.h; derived in DESIGN.md sec. 4, "The conditional fit and limits on the
    signal scale")."""
    return 2 * (_ceil_log2(C) + K) + 14


K_limit = limit_kappa


def _limit_lambda(a, th, mu, muh, thh, lact, d, m, w, log):
    """(lambda, its magnitude) of nusi_plan_response_limit at the conditional optimum (a, th) with counts mu, against the
    best fit (thh, muh): the statistic from ratios, bin by bin, tree(), then the penalties' differences ascending."""
    C = len(d)
    term, mag = np.zeros(C), np.zeros(C)
    for c in range(C):
        dmu = float(mu[c]) - float(muh[c])
        if lact[c]:
            ratio = float(mu[c]) / float(muh[c])
            lr = float(log(ratio)) if ratio > 0.0 else -np.inf
            pl = float(d[c]) * lr
            term[c], mag[c] = dmu - pl, abs(dmu) + abs(pl)
        else:
            term[c], mag[c] = dmu, abs(dmu)
    lam, mg = float(tree(term)), float(tree(mag))
    for j in range(len(th)):
        if w[j] > 0:
            dj = th[j] - thh[j]
            sj = (th[j] - m[j]) + (thh[j] - m[j])
            pd = ((0.5 * w[j]) * dj) * sj
            lam = lam + pd
            mg = mg + abs(pd)
    return lam, mg


def _limit_side(upper, a, zero_ok, s, X, B, d, m, w, ku, klu, hd, S10, muh, thh, lact, log):
    """One side's search of nusi_plan_response_limit from the start a: Newton's iteration in a on lambda(a) = delta / 2,
    a conditional fit per step started from the one before.  zero_ok: the lower side may evaluate a = 0.  Returns (a,
    the side's status word, the last h, eps, g0)."""
    th = [float(v) for v in thh]
    steps, inner, flags, seen, zero_done, aprev = 0, 0, 0, False, False, a
    h = eps = g0 = float("nan")
    while True:
        th, ist, S20 = _fit_fixed_one(a, s, X, B, d, m, w, ku, start=th)
        inner += ist & FIT_STEPS_MASK
        if ist & (FIT_NOT_CONVERGED | FIT_SINGULAR):
            flags |= LIMIT_NOT_CONVERGED
            break
        steps += 1
        mu = a * s
        for j in range(len(th)):
            mu = mu + th[j] * X[j]
        mu = mu + B
        lam, mg = _limit_lambda(a, th, mu, muh, thh, lact, d, m, w, log)
        h = lam - hd
        eps = klu * (mg + hd)
        g0 = S10 - S20
        if not upper and a == 0.0:                  # the one look at zero: the limit is there, or the search goes back
            if not h > 0.0:
                flags |= LIMIT_AT_ZERO
                break
            if steps == LIMIT_ITER_MAX:
                flags |= LIMIT_NOT_CONVERGED
                break
            zero_done, seen, a = True, False, 0.5 * aprev
            continue
        if abs(h) <= eps or (seen and not h > 0.0):
            break
        seen = h > 0.0
        if steps == LIMIT_ITER_MAX:
            flags |= LIMIT_NOT_CONVERGED
            break
        if not (g0 > 0.0 if upper else g0 < 0.0):
            flags |= LIMIT_NOT_CONVERGED
            break
        an = a - h / g0
        if not upper and not an > 0.0:
            seen = False
            if zero_ok and not zero_done:
                aprev, an = a, 0.0
            else:
                an = 0.5 * a
        if not an < np.inf:
            flags |= LIMIT_NOT_CONVERGED
            break
        if an == a:
            break
        a = an
    return a, steps | flags | (min(inner, LIMIT_INNER_MASK) << LIMIT_INNER_SHIFT), h, eps, g0


def limit_host(R, S, data, delta, which="upper", templates=None, prior=None, background=None, log=np.log, details=None):
    """Profile-likelihood limits on the signal's scale, by the search nusi_plan_response_limit defines (include/nusi.h),
    operation for operation: for every table and spectrum the best fit (fit_host; profile_host without templates), and
    the roots a_lo < theta_hat_0 < a_hi of lambda(a) = delta / 2, lambda(a) = min_theta f(a, theta) - min f -- so that
    q(a) = 2 lambda(a) = delta: delta = 2.706 for a one-sided 95 % limit, 1 for a 68 % interval.

    R, S, data, templates (None: K = 0), prior, background, log: as for fit_host.  delta: a finite number > 0.  which:
    "upper", "lower" or "both" (LIMIT_UPPER, LIMIT_LOWER or their sum).  Returns (lo (ntab, Q), hi (ntab, Q), theta_hat
    (ntab, Q, 1 + K), nll_hat (ntab, Q), status (ntab, Q, 3) int32): the best fit's word, then the lower and the upper
    side's -- the outer steps in the low 8 bits, the LIMIT_* flags, the inner Newton steps of all the side's
    conditional fits (saturating at LIMIT_INNER_MASK) from bit LIMIT_INNER_SHIFT.  A side not asked for is NaN with a word
    of 0.  details: None, or a dict that receives 'h', 'eps' and 'g0' (ntab, Q, 2): each side's last lambda - delta / 2,
    its stop's allowance and the derivative there (the tests' bounds), squeezed like the results.  The squeezed axes of events_host are squeezed."""
    s, data, one_tab, one_q = _signal("limit_host", R, S, data)
    ntab, Q, C = s.shape
    wh = {"lower": LIMIT_LOWER, "upper": LIMIT_UPPER, "both": LIMIT_LOWER | LIMIT_UPPER}.get(which, which)
    if wh not in (1, 2, 3):
        raise ValueError("limit_host: which must be 'upper', 'lower' or 'both'")
    delta = float(delta)
    if not np.isfinite(delta) or not delta > 0:
        raise ValueError("limit_host: delta must be finite and > 0")
    K = 0 if templates is None else _templates(templates, C).shape[0]
    T = np.zeros((0, C)) if K == 0 else _templates(templates, C)
    m, w = _prior(K, prior)
    B = np.zeros(C) if background is None else np.array(np.broadcast_to(np.asarray(background, dtype=np.float64), (C,)))
    if K:
        thh, nllh, muh, sth = fit_host(R, S, data, T, prior=prior, background=B, log=log)
    else:
        ah, nllh, muh, sth = profile_host(R, S, data, background=B, log=log)
        thh = np.asarray(ah)[..., None]
    thh, nllh = np.reshape(thh, (ntab, Q, 1 + K)), np.reshape(nllh, (ntab, Q))
    muh, sth = np.reshape(muh, (ntab, Q, C)), np.reshape(sth, (ntab, Q))
    ku, klu, hd = fit_kappa(C, K) * 2.0 ** -53, limit_kappa(C, K) * 2.0 ** -53, 0.5 * delta
    lo, hi = np.full((ntab, Q), np.nan), np.full((ntab, Q), np.nan)
    status = np.zeros((ntab, Q, 3), dtype=np.int32)
    status[..., 0] = sth
    det = {k: np.full((ntab, Q, 2), np.nan) for k in ("h", "eps", "g0")}
    sup_t = np.zeros(C, dtype=bool)                 # a live template supports the bin (a template is never all zeros)
    for j in range(K):
        sup_t |= T[j] > 0
    with np.errstate(all="ignore"):
        for t in range(ntab):
            for q in range(Q):
                x0, ahat = s[t, q], float(thh[t, q, 0])
                S10 = float(tree(x0))
                if sth[t, q] & (FIT_NOT_CONVERGED | FIT_SINGULAR):
                    if wh & LIMIT_LOWER:
                        status[t, q, 1] = LIMIT_NO_FIT
                    if wh & LIMIT_UPPER:
                        status[t, q, 2] = LIMIT_NO_FIT
                    continue
                if S10 == 0.0:
                    if wh & LIMIT_LOWER:
                        lo[t, q], status[t, q, 1] = 0.0, LIMIT_UNBOUNDED | LIMIT_AT_ZERO
                    if wh & LIMIT_UPPER:
                        hi[t, q], status[t, q, 2] = np.inf, LIMIT_UNBOUNDED
                    continue
                mh = muh[t, q]
                lact = (data > 0) & (mh > 0)
                wq = np.where(lact, data / mh, 0.0)
                rq = np.where(lact, wq / mh, 0.0)
                S3 = float(tree((x0 * rq) * x0))
                args = (x0, T, B, data, m[1:], w[1:], ku, klu, hd, S10, mh, thh[t, q, 1:], lact, log)
                # the quadratic model's step, rounded up to a power of two: 2^ceil(e / 2) for delta / S3 = f 2^e, f in [1/2, 1)
                step = float(np.ldexp(1.0, (int(np.frexp(delta / S3)[1]) + 1025) // 2 - 512)) if S3 > 0.0 else hd / S10
                if wh & LIMIT_UPPER:
                    hi[t, q], status[t, q, 2], det["h"][t, q, 1], det["eps"][t, q, 1], det["g0"][t, q, 1] = _limit_side(
                        True, ahat + step, False, *args)
                if wh & LIMIT_LOWER:
                    if ahat == 0.0:
                        lo[t, q], status[t, q, 1] = 0.0, LIMIT_AT_ZERO
                    else:
                        sigonly = bool(np.any((data > 0) & (x0 > 0) & ~(B > 0) & ~sup_t))
                        a = ahat - step
                        if not a > 0.0:
                            a = 0.5 * ahat
                        lo[t, q], status[t, q, 1], det["h"][t, q, 0], det["eps"][t, q, 0], det["g0"][t, q, 0] = _limit_side(
                            False, a, not sigonly, *args)
    if details is not None:
        details.update({k: _squeeze(one_tab, one_q, v)[0] for k, v in det.items()})
    return _squeeze(one_tab, one_q, lo, hi, thh, nllh, status)


def argbest(nll, axis=-1):
    """The selection rule of nusi_plan_response_ensemble (include/nusi.h): along ``axis`` the index of the minimum under
    the key (isnan(nll), nll, index), compared lexicographically -- a NaN loses to everything, +inf included, and equal
    values resolve to the lowest index (all +inf, or all NaN: index 0).  The key is a total order, so any reduction
    tree gives the same index."""
    x = np.asarray(nll, dtype=np.float64)
    if x.ndim == 0 or x.shape[axis] == 0:
        raise ValueError("argbest: nothing to choose from along axis %d of shape %s" % (axis, x.shape))
    nan = np.isnan(x)
    filled = np.where(nan, np.inf, x)
    k = np.argmin(filled, axis=axis)                               # (ties: the first occurrence)
    least = np.take_along_axis(filled, np.expand_dims(k, axis), axis).squeeze(axis)
    # the least is +inf: every non-NaN entry is +inf and the first of THEM wins, not a NaN filled in before it
    return np.where(least == np.inf, np.argmax(~nan, axis=axis), k)


def ensemble_host(R, S, datasets, templates=None, prior=None, background=None, log=np.log):
    """nusi_plan_response_ensemble on the CPU: for every data set p and table t the best spectrum's record.  A loop of
    fit_host (with templates) or profile_host (without: theta has width 1 and holds ahat) over the data sets, reduced
    over the spectra with argbest.

    R: (M, C) or (ntab, M, C).  S: (M,) or (Q, M).  datasets: (C,) or (P, C), entries finite and >= 0.  templates,
    prior, background, log: as for fit_host.  Returns (q (P, ntab) int32, nll (P, ntab), theta (P, ntab, 1 + K),
    status (P, ntab) int32); no axis is squeezed."""
    R = np.asarray(R, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    data = np.asarray(datasets, dtype=np.float64)
    if R.ndim == 2:
        R = R[None]
    if S.ndim == 1:
        S = S[None]
    if data.ndim == 1:
        data = data[None]
    if R.ndim != 3 or S.ndim != 2 or R.shape[1] != S.shape[1]:
        raise ValueError("ensemble_host: R (.., M, C) and S (.., M) do not match: %s, %s" % (R.shape, S.shape))
    ntab, C = R.shape[0], R.shape[2]
    if data.ndim != 2 or data.shape[0] < 1 or data.shape[1] != C:
        raise ValueError("ensemble_host: datasets must have shape (P, %d), P >= 1, got %s" % (C, data.shape))
    if not np.all(np.isfinite(data)) or np.any(data < 0):
        raise ValueError("ensemble_host: a datum is negative or not finite")
    K = 0 if templates is None else _templates(templates, C).shape[0]
    P = data.shape[0]
    q = np.zeros((P, ntab), dtype=np.int32)
    nll, theta, status = np.zeros((P, ntab)), np.zeros((P, ntab, 1 + K)), np.zeros((P, ntab), dtype=np.int32)
    rows = np.arange(ntab)
    for p in range(P):
        if K:
            th, n, _, st = fit_host(R, S, data[p], templates, prior=prior, background=background, log=log)
        else:
            a, n, _, st = profile_host(R, S, data[p], background=background, log=log)
            th = a[..., None]
        best = argbest(n, axis=-1)
        q[p], nll[p], theta[p], status[p] = best, n[rows, best], th[rows, best], st[rows, best]
    return q, nll, theta, status


def order_stat(x, ranks, axis=-1):
    """The band's rule of nusi_plan_response_ensemble_limit (include/nusi.h): along ``axis`` the order statistics of x at
    ``ranks`` (ints, 0 <= r < n, duplicates allowed) under the key (isnan(x), x), ascending -- a NaN sorts after
    everything, +inf included.  The result has the ranks on a new LAST axis in place of ``axis``: shape
    x.shape-without-axis + (len(ranks),).  Entry r is the value with at most r entries before it and more than r before
    or equal to it, so the result does not depend on the order of the input or on how the selection is arranged."""
    x = np.asarray(x, dtype=np.float64)
    r = np.asarray(ranks, dtype=np.int64).reshape(-1)
    if x.ndim == 0 or x.shape[axis] == 0:
        raise ValueError("order_stat: nothing to select from along axis %d of shape %s" % (axis, x.shape))
    n = x.shape[axis]
    if np.any(r < 0) or np.any(r >= n):
        raise ValueError("order_stat: a rank outside 0 .. %d" % (n - 1))
    return np.sort(np.moveaxis(x, axis, -1), axis=-1)[..., r]      # (numpy sorts NaN to the end, behind +inf)


def band_ranks(P, probs=(0.025, 0.16, 0.5, 0.84, 0.975)):
    """The ranks of the quantiles ``probs`` among P toys by the inverted empirical CDF: r = min(P - 1, max(0,
    ceil(f P) - 1)) -- the smallest order statistic with at least a fraction f of the toys at or below it.  The default:
    the median expected limit with its 68 % and 95 % bands.  Returns an int32 array."""
    P = int(P)
    if P < 1:
        raise ValueError("band_ranks: P must be >= 1")
    f = np.asarray(probs, dtype=np.float64).reshape(-1)
    if np.any(~(f >= 0)) or np.any(f > 1):
        raise ValueError("band_ranks: a probability outside [0, 1]")
    return np.minimum(P - 1, np.maximum(0, np.ceil(f * P).astype(np.int64) - 1)).astype(np.int32)


def limit_tally(words):
    """tally[..., side, 4] of nusi_plan_response_ensemble_limit from the side words (..., P, 2): per side the toys whose
    word carries LIMIT_AT_ZERO, LIMIT_UNBOUNDED, LIMIT_NO_FIT and LIMIT_NOT_CONVERGED, in that order (int32)."""
    w = np.asarray(words)
    flags = np.array([LIMIT_AT_ZERO, LIMIT_UNBOUNDED, LIMIT_NO_FIT, LIMIT_NOT_CONVERGED])
    return ((w[..., None] & flags) != 0).sum(axis=-3).astype(np.int32)


def ensemble_limit_host(R, S, datasets, delta, which="upper", ranks=None, templates=None, prior=None, background=None,
                        log=np.log, raw=False):
    """nusi_plan_response_ensemble_limit on the CPU: a loop of limit_host over the data sets, then order_stat over the
    toys and the tally of the side words.

    R: (M, C) or (ntab, M, C).  S: (M,) or (Q, M).  datasets: (C,) or (P, C), entries finite and >= 0.  delta, which,
    templates, prior, background, log: as for limit_host.  ranks: ints in 0 .. P - 1 (None: band_ranks(P)).  Returns
    (band_lo (ntab, Q, NR), band_hi (ntab, Q, NR), tally (ntab, Q, 2, 4) int32) and, with raw, also (lo_all (ntab, Q, P),
    hi_all (ntab, Q, P), words_all (ntab, Q, P, 2) int32); a side not asked for has NaN bands, a tally of 0 and words of
    0.  No axis is squeezed."""
    R = np.asarray(R, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    data = np.asarray(datasets, dtype=np.float64)
    if R.ndim == 2:
        R = R[None]
    if S.ndim == 1:
        S = S[None]
    if data.ndim == 1:
        data = data[None]
    if R.ndim != 3 or S.ndim != 2 or R.shape[1] != S.shape[1]:
        raise ValueError("ensemble_limit_host: R (.., M, C) and S (.., M) do not match: %s, %s" % (R.shape, S.shape))
    ntab, C, Q = R.shape[0], R.shape[2], S.shape[0]
    if data.ndim != 2 or data.shape[0] < 1 or data.shape[1] != C:
        raise ValueError("ensemble_limit_host: datasets must have shape (P, %d), P >= 1, got %s" % (C, data.shape))
    if not np.all(np.isfinite(data)) or np.any(data < 0):
        raise ValueError("ensemble_limit_host: a datum is negative or not finite")
    P = data.shape[0]
    r = band_ranks(P) if ranks is None else np.asarray(ranks, dtype=np.int64).reshape(-1)
    if np.any(r < 0) or np.any(r >= P):
        raise ValueError("ensemble_limit_host: a rank outside 0 .. %d" % (P - 1))
    lo_all, hi_all = np.full((ntab, Q, P), np.nan), np.full((ntab, Q, P), np.nan)
    words = np.zeros((ntab, Q, P, 2), dtype=np.int32)
    for p in range(P):
        lo, hi, _, _, st = limit_host(R, S, data[p], delta, which=which, templates=templates, prior=prior,
                                      background=background, log=log)
        lo_all[..., p], hi_all[..., p] = np.reshape(lo, (ntab, Q)), np.reshape(hi, (ntab, Q))
        words[..., p, :] = np.reshape(st, (ntab, Q, 3))[..., 1:]
    out = (order_stat(lo_all, r), order_stat(hi_all, r), limit_tally(words))
    return out + (lo_all, hi_all, words) if raw else out


def pseudo_data(mu, P, rng):
    """P Poisson pseudo-experiments around the expected counts mu (C,): counts (P, C) as float64, drawn from ``rng``, a
    numpy.random.Generator (the device generates no random numbers: toys are host data)."""
    mu = np.asarray(mu, dtype=np.float64)
    if mu.ndim != 1 or not np.all(np.isfinite(mu)) or np.any(mu < 0):
        raise ValueError("pseudo_data: mu must be a vector of finite expectations >= 0")
    if int(P) < 1:
        raise ValueError("pseudo_data: P must be >= 1")
    return np.ascontiguousarray(rng.poisson(mu, size=(int(P), mu.shape[0])), dtype=np.float64)


# --- the generator of nusi_plan_draw_counts (include/nusi.h "Drawing counts"), operation for operation ---
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
DRAW_INVERSION_MAX, DRAW_PTRS_ROUNDS = 255, 64
DRAW_DATASETS_MAX = 1 << 26    # NUSI_DRAW_DATASETS_MAX
_LOGGAM_A = (8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04,
             8.417508417508418e-04, -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02,
             1.796443723688307e-01, -1.39243221690590e+00)
_M32 = 0xFFFFFFFF


def _philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on Python ints: the four output words."""
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return c0, c1, c2, c3


def philox4x32(counter, key):
    """Philox4x32-10: counter (..., 4) and key (..., 2), 32-bit words (broadcast against each other), to the block
    (..., 4) as uint32.  Ten rounds of c <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key
    bumped by (0x9E3779B9, 0xBB67AE85) after each."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    if c.shape[-1:] != (4,) or k.shape[-1:] != (2,) or np.any(c > _M32) or np.any(k > _M32):
        raise ValueError("philox4x32: counter (..., 4) and key (..., 2) of 32-bit words")
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) for i in range(2))
    m32 = np.uint64(_M32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & m32, (k1 + np.uint64(PHILOX_W1)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniforms(block):
    """The two uniforms in [0, 1) of Philox blocks (..., 4): U0 = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 and U1 the same
    from x2, x3 -- 53 bits each, exact.  Returns (..., 2) float64."""
    x = np.asarray(block, dtype=np.uint64)
    if x.shape[-1:] != (4,) or np.any(x > _M32):
        raise ValueError("uniforms: blocks (..., 4) of 32-bit words")
    hi, lo = x[..., 0::2] >> np.uint64(5), x[..., 1::2] >> np.uint64(6)
    return ((hi << np.uint64(26)) + lo).astype(np.float64) * 2.0 ** -53


def _uniform2(seed, stream, row, p, c, block):
    x = _philox(block, p * 64 + c, row, stream, seed & _M32, (seed >> 32) & _M32)
    return (((x[0] >> 5) << 26) + (x[1] >> 6)) * 2.0 ** -53, (((x[2] >> 5) << 26) + (x[3] >> 6)) * 2.0 ** -53


def loggam(x, log=np.log):
    """numpy's random_loggam as include/nusi.h writes it out: log Gamma(x) for a float x > 0 by a shift up to x0 >= 7,
    ten terms of Stirling's series in 1 / x0^2 (Horner), + 0.5 log 2 pi + (x0 - 0.5) log x0 - x0, and the shift undone
    by subtracting logs; exactly 0 at 1 and 2.  log: a scalar function of a float."""
    x = float(x)
    if x == 1.0 or x == 2.0:
        return 0.0
    n = int(7.0 - x) if x < 7.0 else 0
    x0 = x + float(n)
    ix = 1.0 / x0
    x2 = ix * ix
    gl0 = _LOGGAM_A[9]
    for k in range(8, -1, -1):
        gl0 = gl0 * x2
        gl0 = gl0 + _LOGGAM_A[k]
    gl = gl0 / x0
    gl = gl + 0.5 * 1.8378770664093453
    gl = gl + (x0 - 0.5) * float(log(x0))
    gl = gl - x0
    for _ in range(n):
        x0 = x0 - 1.0
        gl = gl - float(log(x0))
    return gl


def _draw_one(mu, seed, stream, row, p, c, exp, log, rounds=None):
    """One Poisson(mu) count of the identity (seed, stream, row, p, c), as a float.  rounds: None, or a list that
    receives the number of blocks the draw consumed."""
    used = 0
    try:
        if mu == 0.0:
            return 0.0
        if not mu > 0.0 or mu == np.inf:
            return float("nan")
        if mu < 10.0:
            u, _ = _uniform2(seed, stream, row, p, c, 0)
            used = 1
            pk = float(exp(-mu))
            F, k = pk, 0.0
            while not u < F:
                k = k + 1.0
                pk = (pk * mu) / k
                Fn = F + pk
                if (Fn == F and k > mu) or k == float(DRAW_INVERSION_MAX):
                    break
                F = Fn
            return k
        slam, loglam = float(np.sqrt(mu)), float(log(mu))
        b = 0.931 + 2.53 * slam
        a = -0.059 + 0.02483 * b
        invalpha = 1.1239 + 1.1328 / (b - 3.4)
        vr = 0.9277 - 3.6224 / (b - 2.0)
        lia = float(log(invalpha))
        k = 0.0
        for r in range(DRAW_PTRS_ROUNDS):
            u0, V = _uniform2(seed, stream, row, p, c, r)
            used = r + 1
            U = u0 - 0.5
            us = 0.5 - abs(U)
            if us == 0.0:
                continue
            x = (2.0 * a) / us
            x = x + b
            x = x * U
            x = x + mu
            x = x + 0.43
            k = float(np.floor(x))
            if us >= 0.07 and V <= vr:
                return k
            if k < 0.0 or (us < 0.013 and V > us):
                continue
            lhs = (float(log(V)) if V > 0.0 else -np.inf) + lia
            y = a / (us * us)
            y = y + b
            lhs = lhs - float(log(y))
            rhs = -mu + k * loglam
            rhs = rhs - loggam(k + 1.0, log)
            if lhs <= rhs:
                return k
        return k if k > 0.0 else 0.0
    finally:
        if rounds is not None:
            rounds.append(used)


def draw_host(mu, P, seed, stream=0, exp=np.exp, log=np.log, rounds=None):
    """nusi_plan_draw_counts on the CPU: P Poisson counts around every expectation of mu (rows, C) or (C,), by the
    generator include/nusi.h defines, operation for operation -- inversion below mu = 10, Hoermann's PTRS from there, the
    bits from Philox4x32-10 under the key ``seed`` (64 bits) and the counter (block, p 64 + c, row, stream).  Returns
    float64 counts (rows, P, C), or (P, C) for a vector; entry [row, p, c] depends on (seed, stream, row, p, c) and
    mu[row, c] alone.  exp, log: scalar functions of a float (the oracle's ora_exp, ora_log give Plan.draw's integers).
    rounds: None, or a list that receives the blocks each draw consumed, in the output's order."""
    m = np.asarray(mu, dtype=np.float64)
    one = m.ndim == 1
    if one:
        m = m[None]
    if m.ndim != 2 or m.shape[0] < 1 or not 1 <= m.shape[1] <= BINS_MAX:
        raise ValueError("draw_host: mu must have shape (C,) or (rows, C), 1 <= C <= %d, got %s" % (BINS_MAX, m.shape))
    if not np.all(np.isfinite(m)) or np.any(m < 0):
        raise ValueError("draw_host: an expectation is negative or not finite")
    P, seed, stream = int(P), int(seed), int(stream)
    if not 1 <= P <= DRAW_DATASETS_MAX:
        raise ValueError("draw_host: P must be 1 .. %d" % DRAW_DATASETS_MAX)
    if not 0 <= seed < 2 ** 64 or not 0 <= stream < 2 ** 32:
        raise ValueError("draw_host: seed must fit 64 bits and stream 32, unsigned")
    rows, C = m.shape
    out = np.zeros((rows, P, C))
    with np.errstate(all="ignore"):
        for row in range(rows):
            for p in range(P):
                for c in range(C):
                    out[row, p, c] = _draw_one(float(m[row, c]), seed, stream, row, p, c, exp, log, rounds)
    return out[0] if one else out


# --- the generator of nusi_plan_draw_normals (include/nusi.h "Drawing normals"), operation for operation ---
NORMAL_ROUNDS = 64             # NUSI_NORMAL_ROUNDS
NORMAL_BLOCK0 = 0x80000000     # the block word of round 0: the counts use blocks 0 .. 63


def _normal_one(center, sigma, seed, stream, row, p, j, log, rounds=None):
    """One normal variate around ``center`` of width ``sigma``, truncated to x >= 0, of the identity (seed, stream, row,
    p, j), as a float: Marsaglia's polar method, round r on block NORMAL_BLOCK0 + r.  rounds: None, or a list that
    receives the number of blocks the draw consumed."""
    used, x = 0, center
    if sigma != np.inf:
        for r in range(NORMAL_ROUNDS):
            u0, u1 = _uniform2(seed, stream, row, p, j, NORMAL_BLOCK0 + r)
            used = r + 1
            u, v = 2.0 * u0 - 1.0, 2.0 * u1 - 1.0
            uu, vv = u * u, v * v
            sq = uu + vv
            if not sq < 1.0 or sq == 0.0:
                continue
            l2 = -2.0 * float(log(sq))
            f = float(np.sqrt(l2 / sq))
            z = u * f
            sz = sigma * z
            y = center + sz
            if not y >= 0.0:
                continue
            x = y
            break
    if rounds is not None:
        rounds.append(used)
    return x


def draw_normal_host(center, sigma, P, seed, stream=0, log=np.log, rounds=None):
    """nusi_plan_draw_normals on the CPU: P normal variates around every entry of center (rows, J) or (J,), of the widths
    sigma (J,) or a number, truncated to x >= 0, by the rule include/nusi.h defines, operation for operation: round r = 0,
    1, .. takes the uniforms U0, U1 of the Philox block (NORMAL_BLOCK0 + r, p 64 + j, row, stream) under the key ``seed``;
    u = 2 U0 - 1, v = 2 U1 - 1, s = u u + v v, rejected unless 0 < s < 1; x = center + sigma (u sqrt((-2 log s) / s)),
    rejected unless x >= 0; after NORMAL_ROUNDS rejected rounds the draw is the center.  sigma = inf: the center, no bits
    drawn.  The blocks are none of draw_host's (0 .. 63), so the two families are independent under one seed.  Returns
    float64 (rows, P, J), or (P, J) for a vector; entry [row, p, j] depends on (seed, stream, row, p, j), center[row, j]
    and sigma[j] alone.  log: a scalar function of a float (the oracle's ora_log gives Plan.draw_normal's bits).  rounds:
    None, or a list that receives the blocks each draw consumed, in the output's order."""
    c = np.asarray(center, dtype=np.float64)
    one = c.ndim == 1
    if one:
        c = c[None]
    if c.ndim != 2 or c.shape[0] < 1 or not 1 <= c.shape[1] <= BINS_MAX:
        raise ValueError("draw_normal_host: center must have shape (J,) or (rows, J), 1 <= J <= %d, got %s" % (BINS_MAX, c.shape))
    if not np.all(np.isfinite(c)) or np.any(c < 0):
        raise ValueError("draw_normal_host: a center is negative or not finite")
    rows, J = c.shape
    sg = np.array(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (J,)))
    if np.any(np.isnan(sg)) or np.any(sg <= 0):
        raise ValueError("draw_normal_host: a sigma is NaN or not > 0")
    P, seed, stream = int(P), int(seed), int(stream)
    if not 1 <= P <= DRAW_DATASETS_MAX:
        raise ValueError("draw_normal_host: P must be 1 .. %d" % DRAW_DATASETS_MAX)
    if not 0 <= seed < 2 ** 64 or not 0 <= stream < 2 ** 32:
        raise ValueError("draw_normal_host: seed must fit 64 bits and stream 32, unsigned")
    out = np.zeros((rows, P, J))
    with np.errstate(all="ignore"):
        for row in range(rows):
            for p in range(P):
                for j in range(J):
                    out[row, p, j] = _normal_one(float(c[row, j]), float(sg[j]), seed, stream, row, p, j, log, rounds)
    return out[0] if one else out


INJECT_TWO_SIDED, INJECT_UPPER, INJECT_DISCOVERY = 0, 1, 2     # NUSI_INJECT_*
TOYS_FIXED, TOYS_GLOBAL, TOYS_PRIOR = 0, 1, 2                  # NUSI_TOYS_* (NUSI_OPT_TOY_NUISANCE)


def _toys(who, nuisance, allowed):
    ens = {"fixed": TOYS_FIXED, "global": TOYS_GLOBAL, "prior": TOYS_PRIOR}.get(nuisance, nuisance)
    if isinstance(ens, bool) or ens not in allowed:
        raise ValueError("%s: nuisance must be one of %s or the TOYS_* ints" % (
            who, ", ".join(repr(n) for n, v in (("fixed", 0), ("global", 1), ("prior", 2)) if v in allowed)))
    return int(ens)


def _prior_sigma(K, prior, w):
    """The widths (K,) the toys' normals take: sigma_j where template j is constrained (w_j > 0), +inf elsewhere."""
    sg = np.full(K, np.inf)
    if prior is not None and prior[1] is not None:
        sg = np.where(w[1:] > 0, np.broadcast_to(np.asarray(prior[1], dtype=np.float64), (K,)), np.inf)
    return sg


def inject_tally(words):
    """tally[..., 4] of nusi_plan_response_inject from the words (..., P, 2): the toys whose best fit failed
    (FIT_NOT_CONVERGED | FIT_SINGULAR in word 0), whose conditional fit failed (word 1) and whose best fit did not, whose
    best fit ends at theta_hat_0 = 0 (FIT_BOUNDARY | FIT_FLAT) and whose best fit is FIT_INFINITE (int32)."""
    w = np.asarray(words)
    fail = FIT_NOT_CONVERGED | FIT_SINGULAR
    nofit, nocond = (w[..., 0] & fail) != 0, (w[..., 1] & fail) != 0
    cols = [nofit, nocond & ~nofit, (w[..., 0] & (FIT_BOUNDARY | FIT_FLAT)) != 0, (w[..., 0] & FIT_INFINITE) != 0]
    return np.stack([c.sum(axis=-1) for c in cols], axis=-1).astype(np.int32)


def _inject_one(Rt, Sq, at, d, T, prior, B, m, w, md, log):
    """One data set d (C,) through steps 2 - 4 of nusi_plan_response_inject at the test scale ``at``: the best fit
    (fit_host; profile_host without templates), the conditional fit (fit_fixed_host; without templates the single
    evaluation events_host, word 0), lambda by limit_host's rule and the statistic under the mode ``md``.  Returns
    (theta_hat_0, stat, the best fit's word, the conditional fit's, theta_hat (1 + K,), the conditional fit's theta
    (1 + K,), its mu (C,) and lambda's magnitude); a failed best fit: theta_hat_0 and stat are NaN; a failed conditional fit: stat is NaN."""
    fail = FIT_NOT_CONVERGED | FIT_SINGULAR
    if len(T):
        thh, _, muh, sth = fit_host(Rt, Sq, d, T, prior=prior, background=B, log=log)
        thc, _, muc, stc = fit_fixed_host(Rt, Sq, at, d, T, prior=prior, background=B, log=log)
    else:
        ah, _, muh, sth = profile_host(Rt, Sq, d, background=B, log=log)
        thh, thc, stc = np.array([float(ah)]), np.array([at]), 0
        muc = events_host(Rt, Sq, scale=at, background=B)
    lam, mg = _limit_lambda(at, thc[1:], muc, muh, thh[1:], (d > 0) & (muh > 0), d, m[1:], w[1:], log)
    stat, th0 = (2.0 * lam if lam > 0.0 else 0.0), float(thh[0])
    if (md == INJECT_UPPER and th0 > at) or (md == INJECT_DISCOVERY and th0 < at):
        stat = 0.0
    if int(sth) & fail:
        th0 = stat = np.nan
    if int(stc) & fail:
        stat = np.nan
    return th0, stat, int(sth), int(stc), thh, thc, muc, mg


def inject_host(R, S, a_inj, P, seed, theta_inj=None, a_test=None, mode="two-sided", ranks=None, q_obs=None,
                templates=None, prior=None, background=None, exp=np.exp, log=np.log, raw=False, nuisance="fixed"):
    """nusi_plan_response_inject on the CPU: per table t the toys draw_host(mu_inj[t], P, seed, stream=t) around
    mu_inj[t, q] = a_inj[q] s + sum_j theta_inj[j] T_j + B, and per toy a loop of the existing host forms: the best fit
    (fit_host; profile_host without templates), the conditional fit at a_test[q] (fit_fixed_host; without templates the
    single evaluation events_host, word 0), lambda by limit_host's rule and stat = 2 lambda where lambda > 0, else +0.0;
    then order_stat over the toys.

    R: (M, C) or (ntab, M, C).  S: (M,) or (Q, M).  a_inj, a_test (None: a_inj): a number or (Q,), finite and >= 0.
    theta_inj: (K,), None = the prior means.  mode: "two-sided", "upper" (stat = +0.0 where theta_hat_0 > a_test),
    "discovery" (where theta_hat_0 < a_test) or INJECT_*.  ranks: None = band_ranks(P).  q_obs: None, a number or
    (ntab, Q).  templates, prior, background, log: as for fit_host; exp: as for draw_host.  Returns (band_theta (ntab, Q,
    NR), band_stat (ntab, Q, NR), tally (ntab, Q, 4) int32 -- inject_tally), with q_obs also exceed (ntab, Q) int32, the
    toys with stat >= q_obs, and with raw also (theta_all (ntab, Q, P), stat_all (ntab, Q, P), words_all (ntab, Q, P, 2)
    int32, data_all (ntab, Q, P, C)).  A failed best fit: theta_hat_0 and stat are NaN; a failed conditional fit: stat is
    NaN.  No axis is squeezed.

    nuisance: the toys' ensemble (NUSI_OPT_TOY_NUISANCE) for the constrained templates, those with a prior of finite
    width (w_j > 0): "fixed", "global", "prior" or TOYS_*.  "global": per toy the prior means are redrawn, m*_j =
    draw_normal_host(theta_inj, sigma, P, seed, stream=t)[q, p, j]; the counts are "fixed"'s, and the toy's fits and
    lambda take prior = (m*, sigma).  "prior": per toy theta*_j = draw_normal_host(prior means, sigma, P, seed,
    stream=t)[q, p, j] for a constrained template (theta_inj[j] otherwise), the counts are draw_host of a_inj s + sum_j
    theta*_j T_j + B, and the fits take the plan's prior.  With raw and an ensemble other than "fixed" one more array is
    appended: nuis_all (ntab, Q, P, K), the drawn m* or theta*, and the centre where a template is unconstrained.  With K
    = 0 or no constrained template every ensemble gives "fixed"'s values."""
    ens = _toys("inject_host", nuisance, (TOYS_FIXED, TOYS_GLOBAL, TOYS_PRIOR))
    R = np.asarray(R, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    if R.ndim == 2:
        R = R[None]
    if S.ndim == 1:
        S = S[None]
    if R.ndim != 3 or S.ndim != 2 or R.shape[1] != S.shape[1]:
        raise ValueError("inject_host: R (.., M, C) and S (.., M) do not match: %s, %s" % (R.shape, S.shape))
    ntab, C, Q, P = R.shape[0], R.shape[2], S.shape[0], int(P)
    if not 1 <= P:
        raise ValueError("inject_host: P must be >= 1")
    md = {"two-sided": INJECT_TWO_SIDED, "upper": INJECT_UPPER, "discovery": INJECT_DISCOVERY}.get(mode, mode)
    if md not in (0, 1, 2):
        raise ValueError("inject_host: mode must be 'two-sided', 'upper' or 'discovery'")
    K = 0 if templates is None else _templates(templates, C).shape[0]
    T = np.zeros((0, C)) if K == 0 else _templates(templates, C)
    m, w = _prior(K, prior)
    B = np.zeros(C) if background is None else np.array(np.broadcast_to(np.asarray(background, dtype=np.float64), (C,)))
    ai = np.array(np.broadcast_to(np.asarray(a_inj, dtype=np.float64), (Q,)))
    at = ai if a_test is None else np.array(np.broadcast_to(np.asarray(a_test, dtype=np.float64), (Q,)))
    ti = m[1:].copy() if theta_inj is None else np.array(np.broadcast_to(np.asarray(theta_inj, dtype=np.float64), (K,)))
    for v in (ai, at, ti):
        if not np.all(np.isfinite(v)) or np.any(v < 0):
            raise ValueError("inject_host: a_inj, a_test and theta_inj must be finite and >= 0")
    r = band_ranks(P) if ranks is None else np.asarray(ranks, dtype=np.int64).reshape(-1)
    if np.any(r < 0) or np.any(r >= P):
        raise ValueError("inject_host: a rank outside 0 .. %d" % (P - 1))
    s = np.reshape(events_host(R, S), (ntab, Q, C))
    th_all, st_all = np.full((ntab, Q, P), np.nan), np.full((ntab, Q, P), np.nan)
    words, data_all = np.zeros((ntab, Q, P, 2), dtype=np.int32), np.zeros((ntab, Q, P, C))
    sg = _prior_sigma(K, prior, w)
    nuis_all = np.zeros((ntab, Q, P, K))
    with np.errstate(all="ignore"):
        for t in range(ntab):
            if K and ens != TOYS_FIXED:       # (an unconstrained template: sigma = inf, the centre itself)
                centre = ti if ens == TOYS_GLOBAL else np.where(w[1:] > 0, m[1:], ti)
                nuis_all[t] = draw_normal_host(np.broadcast_to(centre, (Q, K)), sg, P, seed, stream=t, log=log)
            if K and ens == TOYS_PRIOR:
                for p in range(P):            # toy p's expectation, every spectrum; its counts are the draw's [q, p]
                    mu_p = ai[:, None] * s[t]
                    for j in range(K):
                        mu_p = mu_p + nuis_all[t, :, p, j][:, None] * T[j][None, :]
                    mu_p = mu_p + B[None, :]
                    for q in range(Q):
                        for c in range(C):
                            data_all[t, q, p, c] = _draw_one(float(mu_p[q, c]), int(seed), t, q, p, c, exp, log)
            else:
                mu_inj = ai[:, None] * s[t]
                for j in range(K):
                    mu_inj = mu_inj + ti[j] * T[j][None, :]
                mu_inj = mu_inj + B[None, :]
                data_all[t] = draw_host(mu_inj, P, seed, stream=t, exp=exp, log=log)
            for q in range(Q):
                for p in range(P):
                    pr_p, m_p = prior, m
                    if K and ens == TOYS_GLOBAL:
                        pr_p = (nuis_all[t, q, p], sg)
                        m_p = _prior(K, pr_p)[0]
                    th0, stat, sth, stc = _inject_one(R[t], S[q], at[q], data_all[t, q, p], T, pr_p, B, m_p, w, md, log)[:4]
                    th_all[t, q, p], st_all[t, q, p], words[t, q, p] = th0, stat, (sth, stc)
    out = (order_stat(th_all, r), order_stat(st_all, r), inject_tally(words))
    if q_obs is not None:
        qo = np.broadcast_to(np.asarray(q_obs, dtype=np.float64), (ntab, Q))
        with np.errstate(invalid="ignore"):
            out = out + ((st_all >= qo[..., None]).sum(axis=-1).astype(np.int32),)
    return out + ((th_all, st_all, words, data_all) + ((nuis_all,) if ens != TOYS_FIXED else ()) if raw else ())


BELT_GRID_MAX = 64                                             # the most grid points of belt_host; its status bits:
BELT_NO_GRID, BELT_NO_FIT, BELT_BAD_POINT, BELT_EMPTY, BELT_LO_EDGE, BELT_HI_EDGE, BELT_GAPS = 1, 2, 4, 8, 16, 32, 64


def belt_accept(exceed, tally, a, alpha, valid, P, flags=0):
    """The acceptance and interval rule of belt_host on arrays.  exceed (..., G) and tally
    (..., G, 4): the counts of P toys a point; a (..., G): the test scales; valid (..., G) bool (or None: all): the
    points whose observed fits held -- the others have no toys; flags (...): the observed side's bits (BELT_NO_GRID,
    BELT_NO_FIT, BELT_BAD_POINT of a failed conditional fit), OR-ed into the word.  nv = P - tally[..., 0] -
    tally[..., 1]; a point is accepted iff it is valid, nv > 0 and float(exceed) > alpha * float(nv), one multiplication
    and one comparison.  Returns (lo (...), hi (...), idx (..., 2) int32, status (...) int32): the first and the last
    accepted grid point and the scales there -- NaN and -1 without one, BELT_EMPTY --, BELT_BAD_POINT where a point has
    nv = 0, BELT_LO_EDGE where idx[0] = 0, BELT_HI_EDGE where idx[1] = G - 1 and BELT_GAPS where a point between the two
    is not accepted.  Nothing is interpolated."""
    ex = np.asarray(exceed)
    ty = np.asarray(tally)
    a = np.asarray(a, dtype=np.float64)
    G = ex.shape[-1]
    if ty.shape != ex.shape + (4,) or a.shape != ex.shape:
        raise ValueError("belt_accept: exceed (..., G), tally (..., G, 4) and a (..., G) do not match")
    ok = np.ones(ex.shape, dtype=bool) if valid is None else np.broadcast_to(np.asarray(valid, dtype=bool), ex.shape)
    nv = int(P) - ty[..., 0].astype(np.int64) - ty[..., 1].astype(np.int64)
    acc = ok & (nv > 0) & (ex.astype(np.float64) > np.float64(alpha) * nv.astype(np.float64))
    nacc = acc.sum(axis=-1)
    first = np.where(nacc > 0, np.argmax(acc, axis=-1), -1)
    last = np.where(nacc > 0, G - 1 - np.argmax(acc[..., ::-1], axis=-1), -1)
    st = np.array(np.broadcast_to(np.asarray(flags, dtype=np.int32), nacc.shape))
    st[np.any(nv <= 0, axis=-1)] |= BELT_BAD_POINT
    st[nacc == 0] |= BELT_EMPTY
    st[first == 0] |= BELT_LO_EDGE
    st[last == G - 1] |= BELT_HI_EDGE
    st[(nacc > 0) & (nacc != last - first + 1)] |= BELT_GAPS
    lo = np.where(nacc > 0, np.take_along_axis(a, np.maximum(first, 0)[..., None], axis=-1)[..., 0], np.nan)
    hi = np.where(nacc > 0, np.take_along_axis(a, np.maximum(last, 0)[..., None], axis=-1)[..., 0], np.nan)
    return lo, hi, np.stack([first, last], axis=-1).astype(np.int32), st.astype(np.int32)


def belt_host(R, S, data, frac, P, seed, ref=None, mode="two-sided", alpha=0.1, templates=None, prior=None, background=None,
              exp=np.exp, log=np.log, raw=False, nuisance="fixed"):
    """The toy-calibrated confidence interval of the signal's scale -- the Feldman-Cousins interval by the profile
    construction -- on a grid of test scales, as a loop of the existing host forms (numpy only; Plan.belt is the device
    call that reproduces it: DESIGN.md sec. 4, "The calibrated interval").  Per table t, spectrum q and grid point g the test
    scale is a = frac[g] * ref[t, q]; the data get inject_host's loop body at a (fit_host / profile_host,
    fit_fixed_host, _limit_lambda), which gives the observed records and q_obs; the toys are draw_host of the conditional
    fit's own mu with stream = t at row q G + g, and each gets the same loop body at a.

    R: (M, C) or (ntab, M, C).  S: (M,) or (Q, M).  data: (C,).  frac: (G,), finite, >= 0, strictly ascending.  ref: None
    (1), a number or (ntab, Q); NaN, infinite or negative: BELT_NO_GRID.  mode: "two-sided", "upper" or INJECT_*.  alpha in
    (0, 1).  templates, prior, background, log: as for fit_host; exp: as for draw_host.  Returns (lo (ntab, Q), hi (ntab,
    Q), idx (ntab, Q, 2) int32, status (ntab, Q) int32, exceed (ntab, Q, G) int32, tally (ntab, Q, G, 4) int32, q_obs
    (ntab, Q, G), theta_obs (ntab, Q, 1 + G, 1 + K), words_obs (ntab, Q, 1 + G) int32) and with raw also (theta_all
    (ntab, Q, G, P), stat_all (ntab, Q, G, P), words_all (ntab, Q, G, P, 2) int32, data_all (ntab, Q, G, P, C)).  A point
    without toys (no grid value, a failed observed fit) has q_obs NaN, counts of 0 and raw outputs of NaN / 0.  No axis
    is squeezed.

    nuisance: "fixed" or "global" (TOYS_FIXED, TOYS_GLOBAL), as for inject_host; "prior" is refused -- the profile
    construction has no such variant.  "global": toy p of a valid point takes prior = (m*, sigma) with m*_j =
    draw_normal_host(centres, sigma, P, seed, stream=t)[q G + g, p, j] for a constrained template, the centre the observed
    conditional fit's theta_j(a), theta_obs[t, q, 1 + g, 1 + j]; the counts are "fixed"'s and the observed pass uses the
    prior as given.  With raw, "global" appends nuis_all (ntab, Q, G, P, K) (0 at a point without toys)."""
    ens = _toys("belt_host", nuisance, (TOYS_FIXED, TOYS_GLOBAL))
    R = np.asarray(R, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    if R.ndim == 2:
        R = R[None]
    if S.ndim == 1:
        S = S[None]
    if R.ndim != 3 or S.ndim != 2 or R.shape[1] != S.shape[1]:
        raise ValueError("belt_host: R (.., M, C) and S (.., M) do not match: %s, %s" % (R.shape, S.shape))
    ntab, C, Q, P = R.shape[0], R.shape[2], S.shape[0], int(P)
    if not 1 <= P:
        raise ValueError("belt_host: P must be >= 1")
    md = {"two-sided": INJECT_TWO_SIDED, "upper": INJECT_UPPER}.get(mode, mode)
    if md not in (INJECT_TWO_SIDED, INJECT_UPPER):
        raise ValueError("belt_host: mode must be 'two-sided' or 'upper'")
    if not 0.0 < alpha < 1.0:
        raise ValueError("belt_host: alpha must lie in (0, 1)")
    fr = np.asarray(frac, dtype=np.float64).reshape(-1)
    G = len(fr)
    if not 1 <= G <= BELT_GRID_MAX or not np.all(np.isfinite(fr)) or np.any(fr < 0) or np.any(np.diff(fr) <= 0):
        raise ValueError("belt_host: frac must hold 1 .. %d finite values >= 0, strictly ascending" % BELT_GRID_MAX)
    d = np.asarray(data, dtype=np.float64).reshape(-1)
    if d.shape != (C,) or not np.all(np.isfinite(d)) or np.any(d < 0):
        raise ValueError("belt_host: data must be (C,), finite and >= 0")
    K = 0 if templates is None else _templates(templates, C).shape[0]
    T = np.zeros((0, C)) if K == 0 else _templates(templates, C)
    m, w = _prior(K, prior)
    B = np.zeros(C) if background is None else np.array(np.broadcast_to(np.asarray(background, dtype=np.float64), (C,)))
    rf = np.array(np.broadcast_to(np.asarray(1.0 if ref is None else ref, dtype=np.float64), (ntab, Q)))
    with np.errstate(invalid="ignore"):
        a = fr[None, None, :] * rf[:, :, None]
        agood = (rf >= 0)[:, :, None] & (a < np.inf)               # (a ref of -1 at frac = 0 gives -0.0: the ref decides)
    fail = FIT_NOT_CONVERGED | FIT_SINGULAR
    q_obs = np.full((ntab, Q, G), np.nan)
    theta_obs, words_obs = np.full((ntab, Q, 1 + G, 1 + K), np.nan), np.zeros((ntab, Q, 1 + G), dtype=np.int32)
    th_all, st_all = np.full((ntab, Q, G, P), np.nan), np.full((ntab, Q, G, P), np.nan)
    words, data_all = np.zeros((ntab, Q, G, P, 2), dtype=np.int32), np.zeros((ntab, Q, G, P, C))
    valid = np.zeros((ntab, Q, G), dtype=bool)
    flags = np.zeros((ntab, Q), dtype=np.int32)
    sg = _prior_sigma(K, prior, w)
    nuis_all = np.zeros((ntab, Q, G, P, K))
    with np.errstate(all="ignore"):
        for t in range(ntab):
            mu_inj = np.zeros((Q, G, C))
            for q in range(Q):
                for g in range(G):
                    at = float(a[t, q, g]) if agood[t, q, g] else 0.0
                    _, stat, sth, stc, thh, thc, muc, _ = _inject_one(R[t], S[q], at, d, T, prior, B, m, w, md, log)
                    theta_obs[t, q, 0], words_obs[t, q, 0] = thh, sth
                    if sth & fail:
                        flags[t, q] |= BELT_NO_FIT
                    if not agood[t, q, g]:
                        flags[t, q] |= BELT_NO_GRID
                        continue
                    theta_obs[t, q, 1 + g], words_obs[t, q, 1 + g] = thc, stc
                    if not sth & fail and stc & fail:
                        flags[t, q] |= BELT_BAD_POINT
                    if not (sth | stc) & fail:
                        valid[t, q, g], q_obs[t, q, g], mu_inj[q, g] = True, stat, muc
            toys = np.reshape(draw_host(mu_inj.reshape(Q * G, C), P, seed, stream=t, exp=exp, log=log), (Q, G, P, C))
            if K and ens == TOYS_GLOBAL:
                centre = np.where(valid[t][..., None], theta_obs[t, :, 1:, 1:], 0.0).reshape(Q * G, K)
                nuis = np.reshape(draw_normal_host(centre, sg, P, seed, stream=t, log=log), (Q, G, P, K))
                nuis_all[t] = np.where(valid[t][..., None, None], nuis, 0.0)
            for q, g in zip(*np.nonzero(valid[t])):
                data_all[t, q, g] = toys[q, g]
                for p in range(P):
                    pr_p, m_p = prior, m
                    if K and ens == TOYS_GLOBAL:
                        pr_p = (nuis_all[t, q, g, p], sg)
                        m_p = _prior(K, pr_p)[0]
                    th0, stat, sth, stc = _inject_one(R[t], S[q], float(a[t, q, g]), toys[q, g, p], T, pr_p, B, m_p, w, md, log)[:4]
                    th_all[t, q, g, p], st_all[t, q, g, p], words[t, q, g, p] = th0, stat, (sth, stc)
    tally = np.where(valid[..., None], inject_tally(words), 0).astype(np.int32)
    with np.errstate(invalid="ignore"):
        exceed = (st_all >= q_obs[..., None]).sum(axis=-1).astype(np.int32)
    out = belt_accept(exceed, tally, a, alpha, valid, P, flags) + (exceed, tally, q_obs, theta_obs, words_obs)
    return out + ((th_all, st_all, words, data_all) + ((nuis_all,) if ens != TOYS_FIXED else ()) if raw else ())


REGION_GRID_MAX = 1024                                         # the most points of composition_belt_host's grid; its status bits:
REGION_NO_FIT, REGION_BAD_POINT, REGION_EMPTY, REGION_ALL = 1, 2, 4, 8


def composition_tally(words):
    """tally[..., 4] of nusi_plan_response_composition_belt from the words (..., P, 2): the toys whose free fit failed
    (FIT_NOT_CONVERGED | FIT_SINGULAR in word 0), whose held fit failed (word 1) and whose free fit did not, whose free
    fit ends with a SIGNAL component at zero (FIT_ZERO << j for a j < 3, FIT_BOUNDARY or FIT_FLAT) and whose free fit is
    FIT_INFINITE (int32)."""
    w = np.asarray(words)
    fail = FIT_NOT_CONVERGED | FIT_SINGULAR
    nofit, nocond = (w[..., 0] & fail) != 0, (w[..., 1] & fail) != 0
    edge = FIT_ZERO | (FIT_ZERO << 1) | (FIT_ZERO << 2) | FIT_BOUNDARY | FIT_FLAT
    cols = [nofit, nocond & ~nofit, (w[..., 0] & edge) != 0, (w[..., 0] & FIT_INFINITE) != 0]
    return np.stack([c.sum(axis=-1) for c in cols], axis=-1).astype(np.int32)


def composition_accept(exceed, tally, valid, alpha, P, q_obs, flags=0):
    """The acceptance rule of composition_belt_host on arrays.  exceed (..., G) and tally (..., G, 4): the counts of P
    toys a point; valid (..., G) bool (or None: all): the points whose observed fits held -- the others have no toys;
    q_obs (..., G); flags (...): the observed side's bits (REGION_NO_FIT, REGION_BAD_POINT of a failed held fit), OR-ed
    into the word.  nv = P - tally[..., 0] - tally[..., 1]; a point is accepted iff it is valid, nv > 0 and float(exceed) >
    alpha * float(nv), one multiplication and one strict comparison.  Returns (accept (..., G) bool, status (...) int32,
    best (...) int32): REGION_BAD_POINT also where a valid point has nv <= 0, REGION_EMPTY where no point is accepted,
    REGION_ALL where there is a valid point and every valid point is accepted; best = the g of the smallest q_obs among
    the valid points, ties to the lowest g, -1 without one.  Nothing is interpolated."""
    ex = np.asarray(exceed)
    ty = np.asarray(tally)
    qo = np.asarray(q_obs, dtype=np.float64)
    if ty.shape != ex.shape + (4,) or qo.shape != ex.shape:
        raise ValueError("composition_accept: exceed (..., G), tally (..., G, 4) and q_obs (..., G) do not match")
    ok = np.ones(ex.shape, dtype=bool) if valid is None else np.broadcast_to(np.asarray(valid, dtype=bool), ex.shape)
    nv = int(P) - ty[..., 0].astype(np.int64) - ty[..., 1].astype(np.int64)
    acc = ok & (nv > 0) & (ex.astype(np.float64) > np.float64(alpha) * nv.astype(np.float64))
    nacc, nok = acc.sum(axis=-1), ok.sum(axis=-1)
    st = np.array(np.broadcast_to(np.asarray(flags, dtype=np.int32), nacc.shape))
    st[np.any(ok & (nv <= 0), axis=-1)] |= REGION_BAD_POINT
    st[nacc == 0] |= REGION_EMPTY
    st[(nok > 0) & (nacc == nok)] |= REGION_ALL
    best = np.where(nok > 0, np.argmin(np.where(ok, qo, np.inf), axis=-1), -1)   # (argmin: the first of equal values)
    return acc, st.astype(np.int32), best.astype(np.int32)


def _composition_one(R3t, Rc, Sq, d, T, prior, B, log):
    """One data set d (C,) through steps 2 - 4 of nusi_plan_response_composition_belt for one table's stack R3t (3, M, C),
    its composed rows Rc (G, M, C) and spectra Sq (Q, M): the free fit (fit_components_host), the held fits (fit_host;
    profile_host without templates), lambda (composition_statistic) and the statistic.  Returns (theta_hat (Q, 3 + K),
    its words (Q,), theta (G, Q, 1 + K), words (G, Q), mu (G, Q, C), stat (G, Q), mag (G, Q)); stat is NaN where either
    word has FIT_NOT_CONVERGED | FIT_SINGULAR."""
    fail = FIT_NOT_CONVERGED | FIT_SINGULAR
    tpl = T if len(T) else None
    thh, _, muh, sth = fit_components_host(R3t[None], Sq, d, templates=tpl, prior=prior, background=B, log=log)
    if len(T):
        th, _, mu, st = fit_host(Rc, Sq, d, T, prior=prior, background=B, log=log)
    else:
        ah, _, mu, st = profile_host(Rc, Sq, d, background=B, log=log)
        th = ah[..., None]
    lam, mag = composition_statistic(mu, th, muh, thh, d, prior=prior if len(T) else None, log=log)
    with np.errstate(invalid="ignore"):
        stat = np.where(lam > 0.0, 2.0 * lam, 0.0)
    stat = np.where(((sth[0][None, :] | st) & fail) != 0, np.nan, stat)
    return thh[0], sth[0], th, st, mu, stat, mag


def composition_belt_host(R3, S, data, phi, P, seed, alpha=0.1, templates=None, prior=None, background=None, exp=np.exp,
                          log=np.log, raw=False):
    """The toy-calibrated confidence region of the source's flavour composition -- the Feldman-Cousins region by the
    profile construction -- on a grid of compositions, as a loop of the existing host forms (numpy only;
    Plan.composition_belt is the device call that reproduces it: DESIGN.md sec. 4, "The composition region").  Per table
    t, spectrum q and grid point g the held rows are response.compose_host(R3, phi)[t, g]; the data get the free fit
    (fit_components_host on R3), the held fit (fit_host on the composed rows; profile_host without templates) and
    composition_statistic, which gives the observed records and q_obs = max(2 lambda, 0); the toys are draw_host of the
    held fit's own mu with stream = t at row q G + g, and each gets the same steps at phi_g.

    R3: (3, M, C) or (ntab, 3, M, C).  S: (M,) or (Q, M).  data: (C,).  phi: (G, 3) or (ntab, G, 3), finite, >= 0, no
    point all zeros, G <= REGION_GRID_MAX.  alpha in (0, 1).  templates, prior, background, log: as for fit_host; exp: as
    for draw_host.  Returns (accept (ntab, Q, G) bool, status (ntab, Q) int32 -- REGION_* --, best (ntab, Q) int32,
    exceed (ntab, Q, G) int32, tally (ntab, Q, G, 4) int32 -- composition_tally --, q_obs (ntab, Q, G), theta_obs (ntab,
    Q, 1 + G, 3 + K): [0] the free fit, [1 + g] the held fit's theta in slots 0 .. K and +0.0 behind, words_obs (ntab, Q,
    1 + G) int32) and with raw also (theta_all (ntab, Q, G, P, 3 + K): the free fit's, NaN where it failed, stat_all
    (ntab, Q, G, P), words_all (ntab, Q, G, P, 2) int32, data_all (ntab, Q, G, P, C)).  A point without toys (a failed
    observed fit) has q_obs NaN, counts of 0 and raw outputs of NaN / 0.  No axis is squeezed."""
    from .response import compose_host
    R3 = np.asarray(R3, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    if R3.ndim == 3:
        R3 = R3[None]
    if S.ndim == 1:
        S = S[None]
    if R3.ndim != 4 or R3.shape[1] != 3 or S.ndim != 2 or R3.shape[2] != S.shape[1]:
        raise ValueError("composition_belt_host: R3 (.., 3, M, C) and S (.., M) do not match: %s, %s" % (R3.shape, S.shape))
    ntab, C, Q, P = R3.shape[0], R3.shape[3], S.shape[0], int(P)
    if not 1 <= P:
        raise ValueError("composition_belt_host: P must be >= 1")
    if not 0.0 < alpha < 1.0:
        raise ValueError("composition_belt_host: alpha must lie in (0, 1)")
    ph = np.asarray(phi, dtype=np.float64)
    if ph.ndim not in (2, 3) or ph.shape[-1] != 3 or (ph.ndim == 3 and ph.shape[0] != ntab):
        raise ValueError("composition_belt_host: phi must have shape (G, 3) or (ntab, G, 3), got %s" % (ph.shape,))
    G = ph.shape[-2]
    if not 1 <= G <= REGION_GRID_MAX or not np.all(np.isfinite(ph)) or np.any(ph < 0) or np.any(np.all(ph == 0, axis=-1)):
        raise ValueError("composition_belt_host: phi must hold 1 .. %d points, finite, >= 0 and none all zeros" % REGION_GRID_MAX)
    d = np.asarray(data, dtype=np.float64).reshape(-1)
    if d.shape != (C,) or not np.all(np.isfinite(d)) or np.any(d < 0):
        raise ValueError("composition_belt_host: data must be (C,), finite and >= 0")
    K = 0 if templates is None else _templates(templates, C).shape[0]
    T = np.zeros((0, C)) if K == 0 else _templates(templates, C)
    B = np.zeros(C) if background is None else np.array(np.broadcast_to(np.asarray(background, dtype=np.float64), (C,)))
    Rc = compose_host(R3, ph)                                   # (ntab, G, M, C)
    fail = FIT_NOT_CONVERGED | FIT_SINGULAR
    NC = 3 + K
    q_obs = np.full((ntab, Q, G), np.nan)
    theta_obs, words_obs = np.zeros((ntab, Q, 1 + G, NC)), np.zeros((ntab, Q, 1 + G), dtype=np.int32)
    th_all, st_all = np.full((ntab, Q, G, P, NC), np.nan), np.full((ntab, Q, G, P), np.nan)
    words, data_all = np.zeros((ntab, Q, G, P, 2), dtype=np.int32), np.zeros((ntab, Q, G, P, C))
    valid = np.zeros((ntab, Q, G), dtype=bool)
    flags = np.zeros((ntab, Q), dtype=np.int32)
    with np.errstate(all="ignore"):
        for t in range(ntab):
            thh, sth, th, st, mu, stat, _ = _composition_one(R3[t], Rc[t], S, d, T, prior, B, log)
            theta_obs[t, :, 0], words_obs[t, :, 0] = thh, sth
            theta_obs[t, :, 1:, :1 + K], words_obs[t, :, 1:] = np.swapaxes(th, 0, 1), st.T
            nofit, nocond = (sth & fail) != 0, (st.T & fail) != 0                    # (Q,), (Q, G)
            flags[t][nofit] |= REGION_NO_FIT
            flags[t][~nofit & nocond.any(axis=1)] |= REGION_BAD_POINT
            valid[t] = ~nofit[:, None] & ~nocond
            q_obs[t] = np.where(valid[t], stat.T, np.nan)
            mu_inj = np.where(valid[t][..., None], np.swapaxes(mu, 0, 1), 0.0)       # (Q, G, C)
            toys = np.reshape(draw_host(mu_inj.reshape(Q * G, C), P, seed, stream=t, exp=exp, log=log), (Q, G, P, C))
            for q, g in zip(*np.nonzero(valid[t])):
                data_all[t, q, g] = toys[q, g]
                for p in range(P):
                    r = _composition_one(R3[t], Rc[t, g:g + 1], S[q:q + 1], toys[q, g, p], T, prior, B, log)
                    if not int(r[1][0]) & fail:
                        th_all[t, q, g, p] = r[0][0]
                    st_all[t, q, g, p], words[t, q, g, p] = r[5][0, 0], (r[1][0], r[3][0, 0])
    tally = np.where(valid[..., None], composition_tally(words), 0).astype(np.int32)
    with np.errstate(invalid="ignore"):
        exceed = (st_all >= q_obs[..., None]).sum(axis=-1).astype(np.int32)
    out = composition_accept(exceed, tally, valid, alpha, P, q_obs, flags) + (exceed, tally, q_obs, theta_obs, words_obs)
    return out + ((th_all, st_all, words, data_all) if raw else ())


def matrix(lo, hi, aeff, migration=None, exposure=1.0):
    """D[c, f, b] = exposure * (hi_b - lo_b) * aeff[f][b] * migration[c][b], shape (C, 3, N).

    lo, hi: the true-energy bin edges [N] (Plan.source_axis()[:2], first N entries); aeff: (3, N) or (N,) (one for
    all flavours), or a callable of (f, E) evaluated at the bins' geometric centres; migration: (C, N), the
    probability of a true-energy bin b event landing in reconstructed bin c (None = the identity, C = N);
    exposure: a number.  ValueError above detector.BINS_MAX reconstructed bins or for a negative or non-finite entry."""
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    if lo.ndim != 1 or lo.shape != hi.shape:
        raise ValueError("matrix: lo and hi must be vectors of one length")
    N = lo.shape[0]
    if callable(aeff):
        E = np.sqrt(lo * hi)
        A = np.array([[float(aeff(f, float(e))) for e in E] for f in range(3)])
    else:
        A = np.broadcast_to(np.asarray(aeff, dtype=np.float64), (3, N))
    mig = np.eye(N) if migration is None else np.asarray(migration, dtype=np.float64)
    if mig.ndim != 2 or mig.shape[1] != N:
        raise ValueError("matrix: migration must have shape (C, %d), got %s" % (N, mig.shape))
    if not 1 <= mig.shape[0] <= BINS_MAX:
        raise ValueError("matrix: %d reconstructed bins, the detector holds 1 .. %d" % (mig.shape[0], BINS_MAX))
    D = (float(exposure) * (hi - lo))[None, None, :] * A[None, :, :] * mig[:, None, :]
    if not np.all(np.isfinite(D)) or np.any(D < 0):
        raise ValueError("matrix: an entry is negative or not finite")
    return np.ascontiguousarray(D)
