"""Parameter points shared by the parity tests (BASELINE.json configs).

Keys are calculate_flux's constructor arguments plus ``source_model``
(0 = the reference's DSNB source, 1 = its commented-out power law).
"""
import numpy as np

MSUM_MIN_NO = 0.0 + np.sqrt(7.42e-5) + np.sqrt(2.514e-3)   # test.py's massless-lightest sum

# test.py -> output/data_massless.txt (the reference's only golden data)
TEST_PY = dict(mphi=5e6, g=1e-6, mntot=MSUM_MIN_NO, si=2.0, norm=6, majorana=True, non_resonant=False,
               normal_ordering=True, N_bins_E=100, lEmin=4, lEmax=9, zmax=5, flav=2, phiphi=False, source_model=0)
# test.cpp (C1), at its own N=100
TEST_CPP = dict(mphi=6e5, g=0.01, mntot=0.1, si=2.5, norm=6, majorana=True, non_resonant=True, normal_ordering=True,
                N_bins_E=100, lEmin=9, lEmax=14, zmax=5, flav=2, phiphi=False, source_model=0)
# C2a: DSNB source with the resonance inside lE 4..9 (N reduced to 100 for the oracle's runtime)
C2A_100 = dict(TEST_CPP, mphi=3e3, g=0.03, lEmin=4, lEmax=9)
# C2b: power-law source at the constructor-default grid
C2B_100 = dict(TEST_CPP, lEmin=12, lEmax=17, source_model=1)

SMALL_CASES = {
    "test_cpp": TEST_CPP,
    "c2a": C2A_100,
    "c2b": C2B_100,
    "dirac": dict(TEST_CPP, majorana=False),
    "inverted": dict(TEST_CPP, mntot=0.2, normal_ordering=False),
    "resonant_only": dict(TEST_CPP, non_resonant=False),
    "flav_e": dict(C2B_100, flav=0),
    "strong": dict(C2B_100, mphi=1e7, g=0.5),
    "test_py": TEST_PY,
}

# full-size BASELINE configs (N_E = 300)
C2A = dict(C2A_100, N_bins_E=300)
C2B = dict(C2B_100, N_bins_E=300)


def oracle_kwargs(kw):
    k = dict(kw)
    k["source"] = k.pop("source_model", 0)
    return k


def scan_points(n_mphi=32, n_g=32, si=2.5, lEmin=12.0, lEmax=17.0, N=300, mphi_range=(5.5, 8.0), g_range=(-3.0, 0.0)):
    """C4: mphi in logspace(5.5, 8, 32) x g in logspace(-3, 0, 32), power-law source."""
    pts = []
    for m in np.logspace(*mphi_range, n_mphi):
        for g in np.logspace(*g_range, n_g):
            pts.append(dict(mphi=float(m), g=float(g), mntot=0.1, si=si, norm=1.0, majorana=True, non_resonant=True,
                            normal_ordering=True, N_bins_E=N, lEmin=lEmin, lEmax=lEmax, zmax=5.0, flav=2,
                            phiphi=False, source_model=1))
    return pts


# Mixed and edge batches of the alpha batch kernel (tests/test_alpha_batch_mixed_gpu.py, the alpha_k_two host check
# in tests/test_hostcheck_tables.py).  Grid N_E = 45, lE 12 -> 12.75 (T = 91: full, diagonal and paired tiles), power-law
# source; couplings from logspace(-3, 0, 9) by index.  The points of one group share (phi-phi, m_phi, masses, majorana,
# non_resonant) -- alpha_batches()'s key -- and so form one batch; A .. E share m_phi, only masses and flags keep them
# apart.  Not in SMALL_CASES: group E's neighbours in g have a NaN oracle flux.
MIXED_GRID = (45, 12.0, 12.75)
MIXED_M1, MIXED_M2 = 10 ** 6.5, 1e8
MIXED_G9 = np.logspace(-3, 0, 9)


def mixed_batch_groups():
    """{group: [points]} -- A: Majorana, NO, mntot 0.1, five couplings, flavour, si and norm varying with the point;
    B: Dirac, the last six couplings (g = 1 among them: warnings 0, .., 0, 2); C: inverted ordering, mntot 0.2;
    D / Dp: Majorana / Dirac resonant-only; E: Majorana with a nearly massless lightest state (mntot = MSUM_MIN_NO:
    state 0 takes the S'+ < 1e-5 Taylor branch everywhere, ~1020 negative alpha entries per table), the five smallest
    couplings (warnings 3, 3, 1, 1, 3) -- at indices 5, 6, 7 (g = 0.075, 0.178, 0.422) the oracle's own flux is NaN
    (Gamma goes negative), at index 8 (g = 1) it is finite but has diverged to -1.6e268; F: Majorana, mntot 0.06,
    m_phi = 1e8, the couplings from index 2 on (warnings 1, 1, 1, 1, 0, 0, 0)."""
    N, lo, hi = MIXED_GRID
    base = scan_points(n_mphi=1, n_g=1, N=N, lEmin=lo, lEmax=hi)[0]

    def grp(idx, **over):
        return [dict(base, mphi=MIXED_M1, g=float(MIXED_G9[i]), **over) for i in idx]
    A = grp([0, 2, 4, 6, 8])
    for k, p in enumerate(A):
        p.update(flav=(0, 1, 2, 0, 1)[k], si=(2.0, 2.25, 2.5, 2.75, 3.0)[k], norm=(1.0, 6.0, 0.5, 2.0, 1.0)[k])
    return {
        "A": A,
        "B": grp(range(3, 9), majorana=False),
        "C": grp([1, 3, 5, 7], mntot=0.2, normal_ordering=False),
        "D": grp([0, 4, 8], non_resonant=False),
        "Dp": grp([2, 5, 7], non_resonant=False, majorana=False),
        "E": grp(range(0, 5), mntot=MSUM_MIN_NO),
        "F": [dict(p, mphi=MIXED_M2) for p in grp(range(2, 9), mntot=0.06)],
    }


# GPU fluxes vs the oracle (north-star bound 1e-9).  The cascade sums in a different order
# (right-looking pushes, multiplied reciprocals, power-law source powers shared along table
# edges): <= 2e-12 observed up to N_E = 1200.
FLUX_RTOL = 1e-11


def rel_err(a, b, floor=1e-280):
    """max |a-b|/|b| over entries with |b| > floor*max|b|; exact agreement required where b == 0."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    zero = b == 0
    if np.any(a[zero] != 0):
        return np.inf
    scale = np.max(np.abs(b)) if b.size else 0.0
    m = np.abs(b) > floor * scale
    if not np.any(m):
        return 0.0
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m])))
