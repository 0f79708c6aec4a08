"""The detector of a plan on the GPU: k_detector_fold (nusi_plan_response_fold, nusi_plan_fold_flux) and
k_detector_events (nusi_plan_response_events).

Yardsticks: nusiprop_amd.detector (numpy).  The fold has no defined summation order; its contract is the bound of
include/nusi.h: every term is non-negative, so any order of K = 3 N products, fused or not, is within gamma_K =
K u / (1 - K u) (u = 2^-53) of the exact sum, and two fp64 evaluations differ by at most 2 gamma_K -- with exact +0.0
where every product is zero.  The events are a defined sum: mu equals detector.events_host bit for bit, and the
statistic differs from detector.poisson_host by the log's last bits only.

Grids (tests/test_tabulated_source_gpu.py): the smallest at which the K remainder, the partial row tile, the partial
column tile and the triangular skip can each go wrong.
  G6   N = 37, M = 43: 3 N = 111 is no multiple of 4, the rows are 2 x 16 + 11, the flavour boundaries fall inside K
       quads, and M > N leaves rows with no zero structure
  G47  N = 45, M = 92
"""
import ctypes

import numpy as np
import pytest

from nusiprop_amd import detector
from tests.test_tabulated_source_gpu import GRIDS, _plan, _pt

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MAXIS = {"G6": 43, "G47": 92}
NTAB = {"G6": 3, "G47": 2}
CS = (1, 5, 16, 17, 64)


@pytest.fixture(scope="module")
def nusi():
    import nusiprop_amd
    nusiprop_amd.load()
    return nusiprop_amd


def _points(grid):
    """Distinct parameter points: the two of the tabulated-source tests and a third coupling."""
    return [_pt(grid, 0, True), _pt(grid, 1, True), _pt(grid, 0, True, g=0.3)][:NTAB[grid]]


_GFLA = {}


def _gfla(nusi, grid):
    """G_fla of the grid's points, computed once and left unchanged."""
    if grid not in _GFLA:
        plan = _plan(nusi, grid, max_points=NTAB[grid], mode="auto")
        _, Gf = plan.response(_points(grid))
        plan.close()
        assert Gf.shape == (NTAB[grid], MAXIS[grid], 3, GRIDS[grid][0])
        assert np.all(np.isfinite(Gf)) and np.all(Gf >= 0) and np.any(Gf > 0)
        assert len({Gf[t].tobytes() for t in range(len(Gf))}) == len(Gf)        # distinct tables
        Gf.setflags(write=False)
        _GFLA[grid] = Gf
    return _GFLA[grid]


def _D(C, N, seed=7, scale=1e3):
    """D (C, 3, N) in [0.5, 2) x scale, one flavour zeroed for one c (flavour 1 of c = 0) and, where there is more than
    one c, the last c zero throughout."""
    rng = np.random.default_rng(seed + 100 * C)
    D = (0.5 + 1.5 * rng.random((C, 3, N))) * scale
    D[0, 1] = 0.0
    if C > 1:
        D[C - 1] = 0.0
    return D


def _B(C, seed=11):
    """A background [C]; 0 for the c that D leaves zero throughout (so mu is exactly 0 there without a source)."""
    B = 0.25 + np.random.default_rng(seed + C).random(C)
    if C > 1:
        B[C - 1] = 0.0
    return B


def _spectra(M, Q, seed=3):
    S = np.random.default_rng(seed + Q).random((Q, M)) * 1e-3
    S[0, 5] = 0.0
    return S


def _products_are_normal(X, D):
    """The bound's condition: every non-zero product is above 1e-280."""
    xmin, dmin = np.min(X[X > 0]), np.min(D[D > 0])
    assert xmin * dmin > 1e-280, (xmin, dmin)


def _check_fold(got, ref, K, what):
    """|got - ref| <= 2 gamma_K ref elementwise, and exactly +0.0 where ref is 0; prints the worst ratio to the bound."""
    assert got.shape == ref.shape
    zero = ref == 0.0
    assert np.all(got[zero] == 0.0) and not np.any(np.signbit(got[zero])), what
    bound = 2 * detector.gamma(K) * ref[~zero]
    ratio = float(np.max(np.abs(got[~zero] - ref[~zero]) / bound)) if np.any(~zero) else 0.0
    print("%s: worst |gpu - host| / (2 gamma_%d host) = %.3f, %d exact zeros" % (what, K, ratio, int(zero.sum())))
    assert ratio <= 1.0, (what, ratio)
    return zero


# --- the fold of response rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("grid", ["G6", "G47"])
def test_fold_of_response_rows(nusi, grid, C):
    Gf = _gfla(nusi, grid)
    N, M = GRIDS[grid][0], MAXIS[grid]
    D = _D(C, N)
    _products_are_normal(Gf, D)
    plan = _plan(nusi, grid)
    plan.set_detector(D, background=_B(C))         # (the response fold adds no background)
    assert plan.detector_bins() == C
    R = plan.fold_response(Gf)
    plan.close()
    assert R.shape == (NTAB[grid], M, C)
    zero = _check_fold(R, detector.fold_host(Gf, D), 3 * N, "%s C=%d response rows" % (grid, C))
    assert np.all(zero[:, 0])                      # row 0 of a response matrix is all zero
    if C > 1:
        assert np.all(zero[:, :, C - 1]) and not np.any(zero[:, 1:, :C - 1])
    # the zeroed flavour: c = 0 equals the fold of G with that flavour removed, within the same bound
    G0 = Gf.copy()
    G0[:, :, 1] = 0.0
    r0 = detector.fold_host(G0, D)[..., 0]
    nz = r0 > 0
    assert np.all(np.abs(R[..., 0][nz] - r0[nz]) <= 2 * detector.gamma(3 * N) * r0[nz])


def test_fold_does_not_read_the_zero_structure(nusi):
    """The contract says the entries of bins b >= n are not read: poisoning them changes no bit."""
    grid, C = "G6", 17
    Gf = _gfla(nusi, grid)
    N, M = GRIDS[grid][0], MAXIS[grid]
    plan = _plan(nusi, grid)
    plan.set_detector(_D(C, N))
    R = plan.fold_response(Gf)
    P = Gf.copy()
    for n0 in range(0, M, 16):                      # a tile of rows n0 .. n0 + 15 reads the bins b < n0 + 16
        P[:, n0:n0 + 16, :, min(N, n0 + 16):] = 1e300
    assert np.array_equal(plan.fold_response(P), R)
    plan.close()


# --- the fold of flux rows ---------------------------------------------------------------------------------------------
_FLUX = {}


def _flux_rows(nusi, n):
    if n not in _FLUX:
        plan = _plan(nusi, "G6", max_points=n, mode="auto")
        _, fla = plan.evolve([_pt("G6", i % 2, True, si=2.0 + 0.05 * i, norm=1.0 + i) for i in range(n)])
        plan.close()
        assert np.all(np.isfinite(fla)) and np.all(fla >= 0) and np.all(np.max(fla, axis=(1, 2)) > 0)
        fla.setflags(write=False)
        _FLUX[n] = fla
    return _FLUX[n]


@pytest.mark.parametrize("C", (5, 64))
@pytest.mark.parametrize("n", (1, 16, 19))
def test_fold_of_flux_rows(nusi, n, C):
    """mu = fold + B: the fold's bound plus one rounding, gamma_{3 N + 1} on either side."""
    fla = _flux_rows(nusi, n)
    N = GRIDS["G6"][0]
    D, B = _D(C, N), _B(C)
    _products_are_normal(fla, D)
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    mu = plan.fold_flux(fla)
    plan.set_detector(D)                           # no background: the plain fold, exact zeros where D is zero
    mu0 = plan.fold_flux(fla)
    plan.close()
    assert mu.shape == (n, C)
    ref0 = detector.fold_host(fla, D)
    _check_fold(mu0, ref0, 3 * N, "G6 C=%d %d flux rows, no background" % (C, n))
    _check_fold(mu, ref0 + B[None, :], 3 * N + 1, "G6 C=%d %d flux rows, background" % (C, n))
    assert np.array_equal(mu[:, C - 1], np.broadcast_to(B[C - 1], (n,)))       # fold 0 + B is B


@pytest.mark.parametrize("grid", ["G6", "G47"])
def test_fold_commutes_with_the_apply(nusi, grid):
    """D . (G_fla . S) = (D . G_fla) . S, the identity the feature rests on: fold_flux of apply_response against events
    of fold_response.  Every term carries at most 3 N + M roundings on either path (a product with S, M - 2 sums over n,
    a product with D, 3 N - 1 sums, the background), so the two agree within 2 gamma_{3 N + M}."""
    Gf = _gfla(nusi, grid)
    N, M, C, Q = GRIDS[grid][0], MAXIS[grid], 17, 5
    D, B, S = _D(C, N), _B(C), _spectra(M, Q)
    plan = _plan(nusi, grid)
    plan.set_detector(D, background=B)
    a = plan.fold_flux(plan.apply_response(Gf, S).reshape(-1, 3, N)).reshape(len(Gf), Q, C)
    b = plan.events(plan.fold_response(Gf), S)
    plan.close()
    assert np.all(b[..., :C - 1] > 0)
    bound = 2 * detector.gamma(3 * N + M) * b
    ratio = float(np.max(np.abs(a - b)[..., :C - 1] / bound[..., :C - 1]))
    print("%s: fold(apply) vs events(fold), worst ratio to 2 gamma_%d: %.3f" % (grid, 3 * N + M, ratio))
    assert np.all(np.abs(a - b) <= bound)
    assert np.array_equal(a[..., C - 1], b[..., C - 1])          # the empty bin: exactly B = 0


# --- events --------------------------------------------------------------------------------------------------------------
_R = {}


def _folded(nusi, C):
    """(R, D, B) on G6: the three tables folded with _D(C), computed once per C and left unchanged."""
    if C not in _R:
        Gf = _gfla(nusi, "G6")
        D, B = _D(C, GRIDS["G6"][0]), _B(C)
        plan = _plan(nusi, "G6")
        plan.set_detector(D, background=B)
        R = plan.fold_response(Gf)
        plan.close()
        R.setflags(write=False)
        _R[C] = (R, D, B)
    return _R[C]


@pytest.mark.parametrize("C", (1, 5, 64))
@pytest.mark.parametrize("Q", (1, 5, 19))
def test_events_equal_the_host_loop(nusi, Q, C):
    R, D, B = _folded(nusi, C)
    S = _spectra(MAXIS["G6"], Q)
    sc = 0.5 + 1.5 * np.random.default_rng(Q).random(Q)
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    mu = plan.events(R, S, scale=sc)
    mu1 = plan.events(R, S)
    plan.close()
    assert mu.shape == (3, Q, C)
    assert np.array_equal(mu, detector.events_host(R, S, scale=sc, background=B))
    assert np.array_equal(mu1, detector.events_host(R, S, background=B))
    assert np.any(mu != mu1)


def _ora_log(oracle_mod):
    L = oracle_mod.lib()
    L.ora_log.restype = ctypes.c_double
    L.ora_log.argtypes = [ctypes.c_double]
    return L.ora_log


def _check_nll(nll, mu, data, log, what):
    """|nll - host| <= 2 (C + 3) u sum_c (mu_c + |data_c log mu_c|): a log within 1 ulp on either side, one product, one
    subtraction and C additions, all of that twice; +inf in the same places."""
    C = len(data)
    host = detector.poisson_host(mu, data, log=log)
    inf = np.isinf(host)
    assert np.array_equal(np.isinf(nll), inf) and np.all(nll[inf] > 0), what
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = np.sum(mu + np.where(data > 0, np.abs(data * np.log(np.where(mu > 0, mu, 1.0))), 0.0), axis=-1)
    bound = 2 * (C + 3) * U * mag
    fin = ~inf
    ratio = float(np.max(np.abs(nll[fin] - host[fin]) / bound[fin])) if np.any(fin) else 0.0
    print("%s: nll vs host, worst ratio to the bound %.3f, bits equal: %s, %d infinite" % (
        what, ratio, np.array_equal(nll, host), int(inf.sum())))
    assert ratio <= 1.0, (what, ratio)
    return host


@pytest.mark.parametrize("C", (1, 5, 64))
def test_statistic(nusi, oracle_mod, C):
    log = _ora_log(oracle_mod)
    R, D, B = _folded(nusi, C)
    Q = 19
    S = _spectra(MAXIS["G6"], Q)
    sc = 0.5 + 1.5 * np.random.default_rng(C).random(Q)
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    mu_only = plan.events(R, S, scale=sc)
    # data near the expectation, some bins empty -- among them the bin the detector never fills (mu = 0 there)
    data = np.floor(mu_only[0, 0] * (0.5 + np.random.default_rng(C + 1).random(C)))
    data[::3] = 0.0
    data[C - 1] = 0.0 if C > 1 else data[0]
    if C == 1:
        data[0] = np.floor(mu_only[0, 0, 0]) + 1.0
    mu, nll = plan.events(R, S, scale=sc, data=data)
    assert np.array_equal(mu, mu_only) and nll.shape == (3, Q)
    host = _check_nll(nll, mu, data, log, "G6 C=%d Q=%d" % (C, Q))
    assert np.all(np.isfinite(host))
    if C > 1:
        assert np.all(mu[..., C - 1] == 0.0)
    # mu_c == 0 < data_c: +inf -- the empty bin with a count (every spectrum), or a spectrum scaled to 0 where the
    # background is 0 too (that spectrum only)
    if C > 1:
        d2 = data.copy()
        d2[C - 1] = 2.0
        _, n2 = plan.events(R, S, scale=sc, data=d2)
        assert np.all(np.isinf(n2)) and np.all(n2 > 0)
        _check_nll(n2, mu, d2, log, "G6 C=%d empty bin with a count" % C)
    plan.set_detector(D)                            # no background
    sc0 = sc.copy()
    sc0[Q // 2] = 0.0
    d3 = np.maximum(data, 1.0)
    d3[C - 1] = 0.0 if C > 1 else 1.0
    mu3, n3 = plan.events(R, S, scale=sc0, data=d3)
    plan.close()
    assert np.all(mu3[:, Q // 2] == 0.0)
    h3 = _check_nll(n3, mu3, d3, log, "G6 C=%d one spectrum scaled to 0" % C)
    assert np.all(np.isinf(h3[:, Q // 2])) and np.all(np.isfinite(np.delete(h3, Q // 2, axis=1)))


@pytest.mark.parametrize("C", (1, 2))
def test_statistic_of_many_spectra_on_few_bins(nusi, oracle_mod, C):
    """A block of k_detector_events owns 4 * 256 / 2^ceil(log2 C) spectra -- 1024 at C = 1, 512 at C = 2 -- more than
    it has threads, so the statistic's pass strides over them; Q = 600 also crosses a block boundary at C = 2.  The
    device form writes into a buffer of NaNs: no entry may be left unwritten."""
    log = _ora_log(oracle_mod)
    R, D, B = _folded(nusi, C)
    Q, M = 600, MAXIS["G6"]
    S = _spectra(M, Q)
    sc = 0.5 + 1.5 * np.random.default_rng(C).random(Q)
    data = np.array([3.0, 0.0][:C])                 # (C = 2: the second bin is the one the detector never fills)
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    mu, nll = plan.events(R, S, scale=sc, data=data)
    assert mu.shape == (3, Q, C) and nll.shape == (3, Q)
    assert np.array_equal(mu, detector.events_host(R, S, scale=sc, background=B))
    host = _check_nll(nll, mu, data, log, "G6 C=%d Q=%d" % (C, Q))
    assert np.all(np.isfinite(host)) and np.all(np.isfinite(nll))
    H = _hip()
    with _Dev(H) as dev:
        dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
        dNll = dev.alloc(nll.nbytes, np.full(nll.shape, np.nan))
        assert plan.events_device(dR, 3, S, None, dNll, scale=sc, data=data) == Q
        assert H.hipDeviceSynchronize() == 0
        assert np.array_equal(dev.fetch(dNll, nll.shape), nll)
    plan.close()


def test_detector_calls_on_several_streams(nusi):
    """One event stands for the end of every detector call of a plan, whatever stream it ran on: an events call on one
    stream, a fold on another, then set_detector (which frees the old detector) and an events call on a third (which
    overwrites the plan's copy of the spectra) -- every result is that of its own inputs."""
    Gf = _gfla(nusi, "G6")
    N, M, C, Q = GRIDS["G6"][0], MAXIS["G6"], 5, 19
    D, D2, B = _D(C, N), _D(C, N, seed=8), _B(C)
    S, S2 = _spectra(M, Q), _spectra(M, Q, seed=4)
    H = _hip()
    H.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    H.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    streams = [ctypes.c_void_p() for _ in range(3)]
    for s in streams:
        assert H.hipStreamCreate(ctypes.byref(s)) == 0
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    R = plan.fold_response(Gf)
    mu = plan.events(R, S)
    try:
        with _Dev(H) as dev:
            dG, dR = dev.alloc(Gf.nbytes, Gf), dev.alloc(R.nbytes, R)
            dMu, dR1, dMu2 = dev.alloc(mu.nbytes), dev.alloc(R.nbytes), dev.alloc(mu.nbytes)
            plan.events_device(dR, 3, S, dMu, stream_ptr=streams[0].value)
            plan.fold_response_device(dG, 3, dR1, stream_ptr=streams[1].value)
            plan.set_detector(D2, background=B)
            plan.events_device(dR, 3, S2, dMu2, stream_ptr=streams[2].value)
            assert H.hipDeviceSynchronize() == 0
            assert np.array_equal(dev.fetch(dMu, mu.shape), mu)
            assert np.array_equal(dev.fetch(dR1, R.shape), R)
            assert np.array_equal(dev.fetch(dMu2, mu.shape), detector.events_host(R, S2, background=B))
    finally:
        for s in streams:
            H.hipStreamDestroy(s)
    plan.close()


# --- results do not depend on neighbours -----------------------------------------------------------------------------
def test_tables_do_not_depend_on_their_neighbours(nusi):
    Gf = _gfla(nusi, "G6")
    N, M, C, Q = GRIDS["G6"][0], MAXIS["G6"], 17, 5
    G20 = np.ascontiguousarray(np.stack([Gf[t % 3] * (1.0 + t / 32.0) for t in range(20)]))
    D, B = _D(C, N), _B(C)
    S = _spectra(M, Q)
    data = np.arange(C, dtype=np.float64) % 4
    data[C - 1] = 0.0
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    R20 = plan.fold_response(G20)
    for t in range(20):
        assert np.array_equal(plan.fold_response(G20[t:t + 1])[0], R20[t]), t
    mu, nll = plan.events(R20[:3], S, scale=2.0, data=data)
    for t in range(3):
        m1, n1 = plan.events(R20[t:t + 1], S, scale=2.0, data=data)
        assert np.array_equal(m1[0], mu[t]) and np.array_equal(n1[0], nll[t]), t
    # ... nor a spectrum on the call's other spectra
    m1, n1 = plan.events(R20[:3], S[3:4], scale=2.0, data=data)
    assert np.array_equal(m1[:, 0], mu[:, 3]) and np.array_equal(n1[:, 0], nll[:, 3])
    plan.close()


# --- surfaces --------------------------------------------------------------------------------------------------------------
def _hip():
    # the HIP runtime libnusi.so itself links (tests/test_response_gpu.py's approach)
    H = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so.7")
    vp = ctypes.c_void_p
    H.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    H.hipFree.argtypes = [vp]
    H.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
    return H


class _Dev:
    """Caller-owned device buffers, freed on exit."""

    def __init__(self, H):
        self.H, self.ptrs = H, []

    def alloc(self, nbytes, src=None):
        p = ctypes.c_void_p()
        assert self.H.hipMalloc(ctypes.byref(p), max(nbytes, 8)) == 0
        self.ptrs.append(p)
        if src is not None:
            assert self.H.hipMemcpy(p, src.ctypes.data, src.nbytes, 1) == 0
        return p.value

    def fetch(self, ptr, shape):
        out = np.zeros(shape)
        assert self.H.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.H.hipFree(p)


def test_device_forms_equal_the_host_forms(nusi):
    Gf = _gfla(nusi, "G6")
    N, M, C, Q = GRIDS["G6"][0], MAXIS["G6"], 17, 5
    fla = _flux_rows(nusi, 19)
    D, D2, B = _D(C, N), _D(C, N, seed=8), _B(C)
    S = _spectra(M, Q)
    data = np.arange(C, dtype=np.float64) % 3
    data[C - 1] = 0.0
    H = _hip()
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    R = plan.fold_response(Gf)
    mu_f = plan.fold_flux(fla)
    mu, nll = plan.events(R, S, scale=1.5, data=data)
    with _Dev(H) as dev:
        dG, dF = dev.alloc(Gf.nbytes, Gf), dev.alloc(fla.nbytes, fla)
        dR, dR2, dMf = dev.alloc(R.nbytes), dev.alloc(R.nbytes), dev.alloc(mu_f.nbytes)
        dMu, dNll = dev.alloc(mu.nbytes), dev.alloc(nll.nbytes)
        plan.fold_response_device(dG, 3, dR)
        plan.fold_flux_device(dF, 19, dMf)
        assert plan.events_device(dR, 3, S, dMu, dNll, scale=1.5, data=data) == Q
        assert H.hipDeviceSynchronize() == 0
        assert np.array_equal(dev.fetch(dR, R.shape), R)
        assert np.array_equal(dev.fetch(dMf, mu_f.shape), mu_f)
        assert np.array_equal(dev.fetch(dMu, mu.shape), mu)
        assert np.array_equal(dev.fetch(dNll, nll.shape), nll)
        # either output alone
        dMu2, dNll2 = dev.alloc(mu.nbytes), dev.alloc(nll.nbytes)
        plan.events_device(dR, 3, S, dMu2, None, scale=1.5)
        plan.events_device(dR, 3, S, None, dNll2, scale=1.5, data=data)
        assert H.hipDeviceSynchronize() == 0
        assert np.array_equal(dev.fetch(dMu2, mu.shape), mu) and np.array_equal(dev.fetch(dNll2, nll.shape), nll)
        # set_detector between two asynchronous calls: the earlier result is the old detector's, the later the new one's
        plan.fold_response_device(dG, 3, dR)
        plan.set_detector(D2, background=B)
        plan.fold_response_device(dG, 3, dR2)
        assert H.hipDeviceSynchronize() == 0
        R2 = plan.fold_response(Gf)
        assert np.array_equal(dev.fetch(dR, R.shape), R)
        assert np.array_equal(dev.fetch(dR2, R.shape), R2) and not np.array_equal(R2, R)
        _check_fold(R2, detector.fold_host(Gf, D2), 3 * N, "G6 C=%d second detector" % C)
    plan.close()


def test_states_and_parameters(nusi):
    from nusiprop_amd import _lib
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    Gf = _gfla(nusi, "G6")
    N, M, C = GRIDS["G6"][0], MAXIS["G6"], 5
    fla = _flux_rows(nusi, 1)
    D, B = _D(C, N), _B(C)
    S = _spectra(M, 2)
    data = np.ones(C)
    R = np.ones((1, M, C))
    plan = _plan(nusi, "G6")

    def refused(code, f, *a, **k):
        with pytest.raises(nusi.NusiError) as ei:
            f(*a, **k)
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    def no_detector():
        assert plan.detector_bins() == 0
        refused(_lib.NUSI_ESTATE, plan.fold_flux, fla)
        refused(_lib.NUSI_ESTATE, plan.fold_response, Gf)
        refused(_lib.NUSI_ESTATE, plan.events, R, S)
        for f, args in ((L.nusi_plan_fold_flux, (None, 1, None, None)), (L.nusi_plan_response_fold, (None, 1, None, None)),
                        (L.nusi_plan_response_events, (None, 1, S.ctypes.data_as(dp), 2, None, None, None, None, None))):
            assert f(plan._h, *args) == _lib.NUSI_ESTATE

    no_detector()                                   # before set_detector
    # set_detector's own refusals leave the plan without a detector
    big = np.ones((65, 3, N))
    assert L.nusi_plan_set_detector(plan._h, 0, D.ctypes.data_as(dp), None) == _lib.NUSI_EPARAM      # C = 0 with D given
    assert L.nusi_plan_set_detector(plan._h, 65, big.ctypes.data_as(dp), None) == _lib.NUSI_EPARAM
    assert L.nusi_plan_set_detector(plan._h, -1, D.ctypes.data_as(dp), None) == _lib.NUSI_EPARAM
    refused(_lib.NUSI_EPARAM, plan.set_detector, big)
    for bad in (-1.0, np.nan, np.inf):
        Db, Bb = D.copy(), B.copy()
        Db[C - 2, 2, N - 1] = bad
        Bb[1] = bad
        refused(_lib.NUSI_EPARAM, plan.set_detector, Db, background=B)
        refused(_lib.NUSI_EPARAM, plan.set_detector, D, background=Bb)
    no_detector()
    plan.set_detector(D, background=B)
    assert plan.detector_bins() == C
    R = plan.fold_response(Gf)
    mu, nll = plan.events(R, S, scale=[1.0, 2.0], data=data)
    # a refused set_detector keeps the detector that is there
    Db = D.copy()
    Db[0, 0, 0] = -1.0
    refused(_lib.NUSI_EPARAM, plan.set_detector, Db)
    assert plan.detector_bins() == C and np.array_equal(plan.fold_response(Gf), R)
    for bad in (-1.0, np.nan, np.inf):
        db, Sb = data.copy(), S.copy()
        db[C - 1] = bad
        Sb[1, M - 1] = bad
        refused(_lib.NUSI_EPARAM, plan.events, R, S, data=db)
        refused(_lib.NUSI_EPARAM, plan.events, R, S, scale=[1.0, bad])
        refused(_lib.NUSI_EPARAM, plan.events, R, Sb)
    H = _hip()
    with _Dev(H) as dev:
        dR, dO = dev.alloc(R.nbytes, R), dev.alloc(mu.nbytes)
        Sp = S.ctypes.data_as(dp)
        ev = L.nusi_plan_response_events
        assert ev(plan._h, dR, 3, Sp, 2, None, data.ctypes.data_as(dp), None, None, None) == _lib.NUSI_EPARAM   # no output
        assert ev(plan._h, dR, 3, Sp, 2, None, None, None, dO, None) == _lib.NUSI_EPARAM                       # nll, no data
        assert ev(plan._h, dR, 0, Sp, 2, None, None, dO, None, None) == _lib.NUSI_EPARAM
        assert ev(plan._h, dR, 3, Sp, 0, None, None, dO, None, None) == _lib.NUSI_EPARAM
        assert L.nusi_plan_fold_flux(plan._h, dR, 0, dO, None) == _lib.NUSI_EPARAM
        assert L.nusi_plan_response_fold(plan._h, None, 1, dO, None) == _lib.NUSI_EPARAM
    m2, n2 = plan.events(R, S, scale=[1.0, 2.0], data=data)         # the refusals changed nothing
    assert np.array_equal(m2, mu) and np.array_equal(n2, nll)
    plan.set_detector(None)                         # cleared
    no_detector()
    plan.set_detector(D)
    assert plan.detector_bins() == C
    assert L.nusi_plan_set_detector(plan._h, 0, None, None) == _lib.NUSI_OK
    no_detector()
    plan.close()
