"""User-tabulated sources for the cascade (numpy only; extension beyond the reference, whose source is fixed at
compile time in Lum(), nuSIprop.hpp:648-662).

A source of the form phi(E') W(z) is described on a plan's grid by two vectors (include/nusi.h,
nusi_plan_set_source):

* ``S[n]``: the integral of the spectrum phi = dN/dE' over bin n of the plan's *source axis*
  (``Plan.source_axis()``), in the source's frame;
* ``w[i]``: the redshift weight W(z_i) in place of the star-formation rate (optional).

A point selects the source in slot k of its plan by ``source_model = tabulated(k)``; its ``norm`` is then an
absolute factor and its ``si`` is ignored.  Typical use::

    lo, hi, z = plan.source_axis()
    plan.set_source(0, sources.broken_power_law(2.0, 3.0, 1e15))        # a callable dN/dE(E)
    plan.set_source(1, sources.power_law_integrals(lo, hi, 2.5), z_weight=lambda z: (1 + z) ** 3)
    flux, fla = plan.evolve([dict(kw, source_model=sources.tabulated(0)), dict(kw, source_model=sources.tabulated(1))])
"""
import numpy as np

SOURCE_TABULATED = 2   # NUSI_SOURCE_TABULATED (include/nusi.h)


def tabulated(slot):
    """The ``source_model`` value of the tabulated source in ``slot`` (>= 0) of a plan."""
    slot = int(slot)
    if slot < 0:
        raise ValueError("source slot must be >= 0")
    return SOURCE_TABULATED + slot


def mixing(normal_ordering=True):
    """|U_fk|^2 of the ordering, shape (3, 3) indexed [flavour e / mu / tau][mass state] (nusi_mixing: the matrix the
    library's flavour fluxes and couplings use)."""
    import ctypes
    from . import _lib
    U2 = np.zeros(9)
    _lib.check(_lib.load().nusi_mixing(1 if normal_ordering else 0, U2.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return U2.reshape(3, 3)


def mass_fractions(flavour, normal_ordering=True):
    """The shares kappa [3] of a source of flavour composition ``flavour`` = (phi_e, phi_mu, phi_tau) emitted into the
    three mass states, kappa_k = sum_f phi_f |U_fk|^2 / sum_f phi_f (nusi_mass_fractions) -- e.g. (1, 2, 0) for pion
    decay, (0, 1, 0) muon-damped, (1, 0, 0) neutron decay.  The kappa of Plan.compose_response / response.compose_host."""
    import ctypes
    from . import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    phi = np.ascontiguousarray(flavour, dtype=np.float64)
    if phi.shape != (3,):
        raise ValueError("mass_fractions: flavour must be (phi_e, phi_mu, phi_tau)")
    kappa = np.zeros(3)
    _lib.check(_lib.load().nusi_mass_fractions(1 if normal_ordering else 0, phi.ctypes.data_as(dp), kappa.ctypes.data_as(dp)))
    return kappa


def bin_integrals(fn, lo, hi, order=12):
    """Integral of ``fn`` (a vectorised callable dN/dE(E)) over each bin [lo[n], hi[n]]: Gauss-Legendre of the
    given order in E, per bin."""
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    x, wq = np.polynomial.legendre.leggauss(int(order))
    half = 0.5 * (hi - lo)
    mid = 0.5 * (hi + lo)
    E = mid[:, None] + half[:, None] * x[None, :]
    f = np.asarray(fn(E), dtype=np.float64)
    return half * np.sum(f * wq[None, :], axis=1)


def power_law_integrals(lo, hi, si, E0=1e14):
    """Closed-form bin integrals of (E / E0)^-si: (hi (hi/E0)^-si - lo (lo/E0)^-si) / (1 - si)  (si != 1)."""
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    si = float(si)
    return (hi * (hi / E0) ** (-si) - lo * (lo / E0) ** (-si)) / (1.0 - si)


def broken_power_law(si_lo, si_hi, E_break, E0=1e14):
    """dN/dE = (E / E0)^-si_lo below E_break and (E_break / E0)^(si_hi - si_lo) (E / E0)^-si_hi above it
    (continuous at the break)."""
    si_lo, si_hi, E_break, E0 = float(si_lo), float(si_hi), float(E_break), float(E0)
    join = (E_break / E0) ** (si_hi - si_lo)

    def fn(E):
        E = np.asarray(E, dtype=np.float64)
        return np.where(E < E_break, (E / E0) ** (-si_lo), join * (E / E0) ** (-si_hi))
    return fn


def exp_cutoff(si, E_cut, E0=1e14):
    """dN/dE = (E / E0)^-si exp(-E / E_cut)."""
    si, E_cut, E0 = float(si), float(E_cut), float(E0)

    def fn(E):
        E = np.asarray(E, dtype=np.float64)
        return (E / E0) ** (-si) * np.exp(-E / E_cut)
    return fn


def spectrum_vector(spectrum, lo, hi):
    """``spectrum`` as the bin-integral vector S [M]: a callable dN/dE(E) is integrated per bin (bin_integrals), an
    array is taken as S itself."""
    if callable(spectrum):
        S = bin_integrals(spectrum, lo, hi)
    else:
        S = np.ascontiguousarray(spectrum, dtype=np.float64)
    if S.shape != (len(lo),):
        raise ValueError("source spectrum: expected %d bin integrals (the source axis), got shape %s" % (len(lo), S.shape))
    return np.ascontiguousarray(S)


def weight_vector(z_weight, z):
    """``z_weight`` as the vector w [Nz] (None stays None: the star-formation rate): a callable of z is evaluated on
    the redshift grid, an array is taken as w itself."""
    if z_weight is None:
        return None
    if callable(z_weight):
        w = np.asarray([z_weight(float(v)) for v in z], dtype=np.float64)
    else:
        w = np.ascontiguousarray(z_weight, dtype=np.float64)
    if w.shape != (len(z),):
        raise ValueError("source redshift weight: expected %d entries (the redshift grid), got shape %s" % (len(z), w.shape))
    return np.ascontiguousarray(w)
