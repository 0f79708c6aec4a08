"""The toy-calibrated region of the flavour composition on the GPU: nusi_plan_response_composition_belt
(k_composition_belt<3 + K>, k_composition_accept) on G6's five tables ("The composition region").

The rows are tests/test_fit_components_gpu.py's: the folded mass-resolved response with its flavour-telling detector,
composed onto the pure flavours.  The data are plan.draw of a signal-plus-background expectation at the composition
(1, 2, 0) / 3.

  * the observed side through existing device code: plan.fit_components and plan.composition_scan, to the bit; q_obs
    within 2 limit_kappa(C, K) u mag of the scan's q (the host's log against the device's: tests/test_belt_gpu.py's
    allowance, mag from composition_statistic);
  * the toys through existing device code: plan.draw of the scan's fixed mu, and on a sample of toys plan.fit_components
    and plan.fit / plan.profile on the composed rows against the toy;
  * against detector.composition_belt_host with the oracle's exp and log (table 0, two spectra, four toys);
  * the counts from the call's own raw arrays and the mask from the counts;
  * every shape again without raw arrays and with OPT_ENSEMBLE_PSLICES in {0, 2}: the same bits;
  * NaN-filled buffers with a tail, each optional output NULL in turn, the device entry on raw pointers;
  * the refusals, by value only.

No call here passes a size that differs from its arrays' own: the size limits are tests/test_composition_belt.py's, on
the CPU, through nusi_composition_belt_shape.
"""
import numpy as np
import pytest

from nusiprop_amd import _lib, detector
from nusiprop_amd.detector import FIT_NOT_CONVERGED, FIT_SINGULAR, REGION_BAD_POINT, REGION_NO_FIT
from nusiprop_amd.response import compose_host
from tests.test_detector_gpu import _Dev, _hip, _spectra
from tests.test_fit_components import triangle
from tests.test_fit_components_gpu import M, _stacks
from tests.test_fit_gpu import _prior_of, _templates
from tests.test_inject_gpu import _ora, _same
from tests.test_profile_gpu import _fetch_int
from tests.test_response_mass_gpu import _plan, nusi  # noqa: F401 (nusi: a fixture)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SEED = 0x5EED0C0DE
ALPHA = 0.1
FAIL = FIT_NOT_CONVERGED | FIT_SINGULAR
NAMES = ("accept", "status", "best", "exceed", "tally", "q_obs", "theta_obs", "words_obs", "theta_all", "stat_all",
         "words_all", "data_all")
INTS = (0, 1, 2, 3, 4, 7, 10)
TAIL = 64


def _phi(G):
    """1: pion decay; 4: it, a vertex, an unnormalised interior point, the democratic one; 21: the triangle at step 0.2
    (its three vertices, where two phi are exactly 0) with one point repeated."""
    if G == 1:
        return np.array([[1.0, 2.0, 0.0]]) / 3.0
    if G == 4:
        return np.array([[1.0 / 3.0, 2.0 / 3.0, 0.0], [0.0, 0.0, 1.0], [0.4, 0.1, 0.25], [1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0]])
    phi = triangle(5)
    assert len(phi) == 21 and G == 21
    phi[7] = phi[3]
    return phi


def _setting(nusi, C, K, kind, Q):  # noqa: F811
    """(plan, R3, S, T, prior, B, data): the pure-flavour stack; the data drawn around 120 signal events of spectrum 0 in
    table 0's fullest bin at the composition (1, 2, 0) / 3, on the templates at 1 and the background."""
    _, pure, D, B = _stacks(nusi, C)
    R3 = np.ascontiguousarray(pure)
    S = _spectra(M, Q)
    T = _templates(C, K, scale=20.0) if K else None
    prior = _prior_of(T, kind) if K else None
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    if K:
        plan.set_templates(T, prior=prior)
    s = detector.events_host(plan.compose_response(R3[:1], np.array([1.0, 2.0, 0.0]) / 3.0), S[:1])[0, 0]
    mean = (120.0 / s.max() if s.max() > 0 else 0.0) * s + B
    if K:
        mean = mean + T.sum(axis=0)
    data = plan.draw(mean, 1, SEED + 1)[0]
    return plan, R3, S, T, prior, B, data


def _call(plan, R3, S, data, phi, P, raw=True):
    return plan.composition_belt(R3, S, data, phi, P, SEED, alpha=ALPHA, raw=raw)


def _valid_flags(words_obs):
    nofit = (words_obs[..., 0] & FAIL) != 0
    nocond = (words_obs[..., 1:] & FAIL) != 0
    flags = np.where(nofit, REGION_NO_FIT, 0) | np.where((~nofit[..., None] & nocond).any(-1), REGION_BAD_POINT, 0)
    return ~nofit[..., None] & ~nocond, flags.astype(np.int32)


def _allow(C, K, mag):
    return 2.0 * detector.limit_kappa(C, K) * U * mag


def _composed(plan, R3, phi):
    return plan.compose_response(R3, phi)                           # (ntab, G, M, C)


def _held(plan, K, R, S, d):
    if K:
        th, _, mu, st = plan.fit(R, S, d)
        return th, mu, st
    ah, _, mu, st = plan.profile(R, S, d)
    return ah[..., None], mu, st


def _observed_through_device_calls(plan, R3, S, K, prior, data, phi, out, what):
    """theta_obs[..., 0] = plan.fit_components, theta_obs[..., 1 + g] = composition_scan's fixed records, q_obs against its
    q.  Returns the scan's fixed mu (ntab, G, Q, C)."""
    q_obs, th_obs, w_obs = out[5:8]
    C = R3.shape[3]
    free = plan.fit_components(R3, S, data)
    assert np.array_equal(th_obs[:, :, 0], free[0]) and np.array_equal(w_obs[:, :, 0], free[3]), what
    q, fixed, free2, word = plan.composition_scan(R3, S, data, phi, prior=prior)
    assert np.array_equal(th_obs[:, :, 1:, :1 + K], np.swapaxes(fixed[0], 1, 2)), what
    assert np.all(th_obs[:, :, 1:, 1 + K:] == 0.0) and not np.any(np.signbit(th_obs[:, :, 1:, 1 + K:])), what
    assert np.array_equal(w_obs[:, :, 1:], np.swapaxes(fixed[3], 1, 2)), what
    valid, _ = _valid_flags(w_obs)
    assert np.array_equal(np.isnan(q_obs), ~valid), what
    with np.errstate(all="ignore"):
        _, mag = detector.composition_statistic(fixed[2], fixed[0], free[2][:, None], free[0][:, None], data, prior=prior)
    qs, mg = np.swapaxes(q, 1, 2), np.swapaxes(mag, 1, 2)
    fin = valid & np.isfinite(qs) & np.isfinite(mg)
    assert np.all(q_obs[valid] >= 0) and not np.any(np.signbit(q_obs[valid])), what
    err, allow = np.abs(q_obs[fin] - qs[fin]), _allow(C, K, mg[fin])
    assert np.all(err <= allow), (what, float(err.max()), np.argwhere(fin)[np.argmax(err - allow)])
    worst = float(np.max(err / np.where(allow > 0, allow, 1.0))) if err.size else 0.0
    print("%s: %d observed records through composition_scan, |q_obs - q| / allowance max %.3f, %d bit-equal" % (
        what, int(fin.sum()), worst, int(np.count_nonzero(q_obs[fin] == qs[fin]))))
    return fixed[2]


def _toys_through_device_calls(plan, R3, Rc, S, K, prior, mu_fixed, P, out, what):
    """data_all = plan.draw of the scan's fixed mu (stream = t, row = q G + g); on a sample of toys theta_all and the words
    equal plan.fit_components and plan.fit / plan.profile against the toy, stat within the allowance."""
    q_obs, w_obs = out[5], out[7]
    th_all, st_all, words, toys = out[8:]
    ntab, Q, G = q_obs.shape
    C = R3.shape[3]
    valid, _ = _valid_flags(w_obs)
    n = 0
    for t in sorted({0, ntab - 2}):
        mu_inj = np.where(valid[t][..., None], np.swapaxes(mu_fixed[t], 0, 1), 0.0).reshape(Q * G, C)
        want = plan.draw(mu_inj, P, SEED, stream=t).reshape(Q, G, P, C)
        assert np.array_equal(toys[t], want), (what, t)
        for q in sorted({0, Q - 1}):
            for g in sorted({0, G // 2, G - 1}):
                if not valid[t, q, g]:
                    continue
                for p in range(min(P, 3)):
                    d = toys[t, q, g, p]
                    fth, _, fmu, fst = (x[0, 0] for x in plan.fit_components(R3[t:t + 1], S[q:q + 1], d))
                    hth, hmu, hst = (x[0, 0] for x in _held(plan, K, Rc[t, g][None], S[q:q + 1], d))
                    assert words[t, q, g, p].tolist() == [int(fst), int(hst)], (what, t, q, g, p)
                    if int(fst) & FAIL:
                        assert np.all(np.isnan(th_all[t, q, g, p]))
                    else:
                        assert np.array_equal(th_all[t, q, g, p], fth), (what, t, q, g, p)
                    if (int(fst) | int(hst)) & FAIL:
                        assert np.isnan(st_all[t, q, g, p])
                        continue
                    with np.errstate(all="ignore"):
                        lam, mag = detector.composition_statistic(hmu, hth, fmu, fth, d, prior=prior)
                    stat = max(2.0 * float(lam), 0.0)
                    if np.isfinite(stat) and np.isfinite(mag):
                        assert abs(st_all[t, q, g, p] - stat) <= _allow(C, K, float(mag)), (what, t, q, g, p, st_all[t, q, g, p], stat)
                    n += 1
    print("%s: %d toys' records equal plan.fit_components and plan.fit / profile against the toy" % (what, n))


def _against_host_form(R3, S, T, prior, B, data, phi, P, out, exp, log, what):
    K, C, nq, np_ = (0 if T is None else len(T)), R3.shape[3], min(len(S), 2), min(P, 4)
    h = detector.composition_belt_host(R3[0], S[:nq], data, phi, np_, SEED, alpha=ALPHA, templates=T, prior=prior, background=B,
                                       exp=exp, log=log, raw=True)
    flags = ~(detector.FIT_STEPS_MASK | (detector.FIT_TRIALS_MASK << detector.FIT_TRIALS_SHIFT))
    got = [x[0:1, :nq] for x in out]
    got[8], got[9], got[10], got[11] = (x[:, :, :, :np_] for x in got[8:])
    assert np.array_equal(h[11], got[11]), what                       # the toys
    assert np.array_equal(h[6], got[6], equal_nan=True), what         # theta_obs
    assert np.array_equal(h[8], got[8], equal_nan=True), what         # theta_hat of every toy
    assert np.array_equal(h[7] & flags, got[7] & flags) and np.array_equal(h[10] & flags, got[10] & flags), what
    # exceed and tally of the toys both sides ran: the device's from its own raw arrays
    with np.errstate(invalid="ignore"):
        assert np.array_equal(h[3], (got[9] >= got[5][..., None]).sum(-1)), what
    assert np.array_equal(h[4], detector.composition_tally(got[10])), what
    if np_ == P:
        assert np.array_equal(h[3], got[3]) and np.array_equal(h[4], got[4]), what
    Rc = compose_host(R3[:1], phi)[0]
    same = total = 0
    for hx, gx, toy in ((h[5], got[5], False), (h[9], got[9], True)):
        assert np.array_equal(np.isnan(hx), np.isnan(gx)), what
        for i in zip(*np.nonzero(~np.isnan(hx))):
            total += 1
            if hx[i] == gx[i]:
                same += 1
                continue
            q, g = i[1], i[2]
            d = got[11][i] if toy else data
            mg = detector._composition_one(R3[0], Rc[g:g + 1], S[q:q + 1], d, np.zeros((0, C)) if T is None else T, prior, B, log)[6]
            assert abs(hx[i] - gx[i]) <= _allow(C, K, float(mg[0, 0])), (what, i, hx[i], gx[i])
    print("%s: %d of %d statistics (q_obs and stat) equal the host form's to the bit" % (what, same, total))


def _every_way(nusi, oracle_mod, C, K, kind, Q, G, P):  # noqa: F811
    exp, log = _ora(oracle_mod)
    what = "G6 C=%d K=%d prior %s Q=%d G=%d P=%d" % (C, K, kind, Q, G, P)
    plan, R3, S, T, prior, B, data = _setting(nusi, C, K, kind, Q)
    try:
        ntab, phi = R3.shape[0], _phi(G)
        base = _call(plan, R3, S, data, phi, P)
        assert len(base) == 12 and base[0].dtype == bool and all(base[k].dtype == np.int32 for k in INTS[1:])
        assert base[0].shape == (ntab, Q, G) and base[6].shape == (ntab, Q, 1 + G, 3 + K)
        assert base[8].shape == (ntab, Q, G, P, 3 + K) and base[11].shape == (ntab, Q, G, P, C)
        valid, flags = _valid_flags(base[7])
        # a point without toys: NaN / 0
        for k in (5, 8, 9):
            assert np.all(np.isnan(base[k][~valid])), (what, NAMES[k])
        for k in (0, 3, 4, 10, 11):
            assert not np.any(base[k][~valid]), (what, NAMES[k])
        mu_fixed = _observed_through_device_calls(plan, R3, S, K, prior, data, phi, base, what)
        Rc = _composed(plan, R3, phi)
        _toys_through_device_calls(plan, R3, Rc, S, K, prior, mu_fixed, P, base, what)
        _against_host_form(R3, S, T, prior, B, data, phi, P, base, exp, log, what)
        # the counts from the raw arrays, the mask from the counts
        with np.errstate(invalid="ignore"):
            exceed = (base[9] >= base[5][..., None]).sum(-1).astype(np.int32)
        tally = np.where(valid[..., None], detector.composition_tally(base[10]), 0).astype(np.int32)
        assert np.array_equal(exceed, base[3]) and np.array_equal(tally, base[4]), what
        _same(base[:3], detector.composition_accept(exceed, tally, valid, ALPHA, P, base[5], flags), what + ": the mask from the counts",
              NAMES[:3])
        nofit = (base[1] & REGION_NO_FIT) != 0
        ntoys = max(int(valid.sum()) * P, 1)
        print("%s: %d of %d points valid, %d accepted, %d of %d pairs NO_FIT; %.1f %% of the toys end with a signal component "
              "at zero, %.2f %% free fits failed" % (what, int(valid.sum()), valid.size, int(base[0].sum()), int(nofit.sum()),
                                                    nofit.size, 100.0 * base[4][..., 2].sum() / ntoys,
                                                    100.0 * base[4][..., 0].sum() / ntoys))
        # every slicing: the same bits, with and without the raw arrays
        for ps in (0, 2):
            plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, ps)
            tag = "%s: p-slices %d" % (what, ps)
            _same(_call(plan, R3, S, data, phi, P, raw=False), base[:8], tag + ", no raw arrays", NAMES[:8])
            if ps:
                _same(_call(plan, R3, S, data, phi, P), base, tag + ", raw arrays", NAMES)
        plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, 0)
    finally:
        plan.close()


CLASSES = [(C, K, kind) for C in (1, 5, 17, 64) for K, kind in ((0, "none"), (1, "none"), (3, "none"), (3, "mixed"))]
SHAPES = [(1, 1, 1), (3, 21, 33), (1, 21, 5), (3, 1, 33)]


@pytest.mark.parametrize("C,K,kind", CLASSES)
def test_region_on_the_real_fold(nusi, oracle_mod, C, K, kind):  # noqa: F811
    _every_way(nusi, oracle_mod, C, K, kind, 3, 4, 5)


@pytest.mark.parametrize("C,K,kind,Q,G,P", [(C, K, kind) + SHAPES[(i + j) % 4]
                                            for i, C in enumerate((1, 5, 17, 64))
                                            for j, (K, kind) in enumerate(((0, "none"), (1, "none"), (3, "mixed")))])
def test_region_shapes(nusi, oracle_mod, C, K, kind, Q, G, P):  # noqa: F811
    """One record in all; the triangle at step 0.2 with its vertices and a repeated point -- several row blocks a table
    and a partial last one (63 rows in blocks of 4 at C = 64, of 8 at C = 17) --; one spectrum; one point."""
    _every_way(nusi, oracle_mod, C, K, kind, Q, G, P)


def test_phi_per_table(nusi):  # noqa: F811
    """phi (ntab, G, 3): each table's own grid; equal to the calls with that table alone."""
    C, K, Q, G, P = 5, 1, 3, 4, 5
    plan, R3, S, T, prior, B, data = _setting(nusi, C, K, "mixed", Q)
    try:
        ntab = R3.shape[0]
        phi = np.stack([np.roll(_phi(G), t, axis=0) * (1.0 + 0.25 * t) for t in range(ntab)])
        out = _call(plan, R3, S, data, phi, P)
        one = _call(plan, R3, S, data, phi[0], P)
        _same([x[:1] for x in out], [x[:1] for x in one], "table 0", NAMES)
        assert not np.array_equal(out[5][1], one[5][1])
        q = plan.composition_scan(R3, S, data, phi, prior=prior)[1][0]
        assert np.array_equal(out[6][:, :, 1:, :1 + K], np.swapaxes(q, 1, 2))
    finally:
        plan.close()


def test_the_device_form_buffers_and_refusals(nusi):  # noqa: F811
    """Every size passed here is its array's own: the refusal cases vary values only."""
    C, K, Q, G, P = 17, 3, 3, 4, 5
    plan, R3, S, T, prior, B, data = _setting(nusi, C, K, "mixed", Q)
    H = _hip()
    try:
        ntab, phi = R3.shape[0], _phi(G)
        base = list(_call(plan, R3, S, data, phi, P))
        base[0] = base[0].astype(np.int32)
        keys = ["d_%s_ptr" % n for n in NAMES]
        needs = {"exceed", "tally", "q_obs", "words_obs"}
        with _Dev(H) as dev:
            dR = dev.alloc(R3.nbytes, R3)
            for skip in (None,) + NAMES:
                bufs = []
                for k, x in enumerate(base):
                    fill = np.full(x.size + TAIL, -1, dtype=np.int32) if k in INTS else np.full(x.size + TAIL, np.nan)
                    bufs.append(dev.alloc(fill.nbytes, fill))
                args = {keys[k]: None if NAMES[k] == skip else bufs[k] for k in range(12)}
                if skip in needs:                                   # the mask needs it: without the mask, then
                    for k in range(3):
                        args[keys[k]] = None
                assert plan.composition_belt_device(dR, ntab, S, data, phi, P, SEED, alpha=ALPHA, **args) == (Q, G)
                assert H.hipDeviceSynchronize() == 0
                for k, x in enumerate(base):
                    n = x.size + TAIL
                    got = _fetch_int(H, bufs[k], (n,)) if k in INTS else dev.fetch(bufs[k], (n,))
                    empty = np.all(got[x.size:] == -1) if k in INTS else np.all(np.isnan(got[x.size:]))
                    assert empty, (skip, NAMES[k], "written behind the last element")
                    if NAMES[k] == skip or (skip in needs and k < 3):
                        assert np.all(got == -1) if k in INTS else np.all(np.isnan(got)), (skip, NAMES[k])
                    else:
                        assert np.array_equal(got[:x.size].reshape(x.shape), x, equal_nan=True), (skip, NAMES[k])
            # refusals change nothing
            dA = dev.alloc(base[5].nbytes, np.full(base[5].shape, np.nan))
            ok = dict(alpha=ALPHA, d_q_obs_ptr=dA)
            neg, nan_ = data.copy(), data.copy()
            neg[0], nan_[C - 1] = -1.0, np.nan
            p_nan, p_neg, p_zero = phi.copy(), phi.copy(), phi.copy()
            p_nan[1, 0], p_neg[2, 1], p_zero[3] = np.nan, -0.25, 0.0
            p_inf = phi.copy()
            p_inf[0, 2] = np.inf
            dI = dev.alloc(base[0].nbytes, base[0])
            bad = [dict(ok, alpha=0.0), dict(ok, alpha=1.0), dict(ok, alpha=np.nan), dict(ok, phi_=p_nan), dict(ok, phi_=p_neg),
                   dict(ok, phi_=p_zero), dict(ok, phi_=p_inf), dict(ok, data_=neg), dict(ok, data_=nan_), dict(alpha=ALPHA),
                   dict(ok, d_accept_ptr=dI), dict(ok, d_status_ptr=dI, d_tally_ptr=dI, d_words_obs_ptr=dI),
                   dict(ok, d_best_ptr=dI, d_exceed_ptr=dI, d_tally_ptr=dI)]
            for b in bad:
                b = dict(b)
                fb, db = b.pop("phi_", phi), b.pop("data_", data)
                with pytest.raises(_lib.NusiError) as e:
                    plan.composition_belt_device(dR, ntab, S, db, fb, P, SEED, **b)
                assert e.value.code == _lib.NUSI_EPARAM, b
            with pytest.raises(_lib.NusiError) as e:
                plan.composition_belt_device(0, ntab, S, data, phi, P, SEED, **ok)
            assert e.value.code == _lib.NUSI_EPARAM
            Sbad = S.copy()
            Sbad[0, 3] = -1.0
            with pytest.raises(_lib.NusiError) as e:
                plan.composition_belt_device(dR, ntab, Sbad, data, phi, P, SEED, **ok)
            assert e.value.code == _lib.NUSI_EPARAM
            # GLOBAL with a constrained template; without one, and under FIXED, the call runs
            plan.set_option(_lib.OPT_TOY_NUISANCE, _lib.TOYS_GLOBAL)
            with pytest.raises(_lib.NusiError) as e:
                plan.composition_belt_device(dR, ntab, S, data, phi, P, SEED, **ok)
            assert e.value.code == _lib.NUSI_EPARAM and "NUSI_OPT_TOY_NUISANCE" in _lib.last_error()
            assert H.hipDeviceSynchronize() == 0
            assert np.all(np.isnan(dev.fetch(dA, base[5].shape)))
            assert np.array_equal(_fetch_int(H, dI, base[0].shape), base[0])
            plan.set_templates(T)
            free = _call(plan, R3, S, data, phi, P)
            plan.set_option(_lib.OPT_TOY_NUISANCE, _lib.TOYS_FIXED)
            _same(_call(plan, R3, S, data, phi, P), free, "no constrained template: GLOBAL is FIXED", NAMES)
            plan.set_templates(T, prior=prior)
            again = list(_call(plan, R3, S, data, phi, P))
            again[0] = again[0].astype(np.int32)
            _same(again, base, "after the refusals", NAMES)
        plan.set_detector(None)
        with pytest.raises(_lib.NusiError) as e:
            plan.composition_belt(R3, S, data, phi, P, SEED)
        assert e.value.code == _lib.NUSI_ESTATE
    finally:
        plan.close()
