"""Batched parameter scans on one GPU: a thin wrapper of the nusi_plan C API.

A Plan fixes the energy/redshift grid (N_bins_E, lEmin, lEmax, zmax) of the
reference's constructor (nuSIprop.hpp:113-128) and holds the Stage-A tables of
up to ``max_points`` parameter points in HBM.  ``evolve`` runs, on the GPU,
exactly what calculate_flux::evolve() does for each point (nuSIprop.hpp:176-337).
"""
import ctypes

import numpy as np

from . import _lib


def params_array(points, grid_args=None):
    """ctypes array of struct nusi_params; dict points may omit the grid keys
    when grid_args = (N_bins_E, lEmin, lEmax, zmax) is given."""
    arr = (_lib.NusiParams * len(points))()
    for k, p in enumerate(points):
        if isinstance(p, _lib.NusiParams):
            arr[k] = p
        else:
            q = dict(p)
            if grid_args is not None:
                for key, v in zip(("N_bins_E", "lEmin", "lEmax", "zmax"), grid_args):
                    q.setdefault(key, v)
            arr[k] = _lib.make_params(**q)
    return arr


class Plan:
    def __init__(self, N_bins_E=300, lEmin=12.0, lEmax=17.0, zmax=5.0, max_points=1, device=0, reference_order=None):
        """reference_order: None = the library default (the reference's own arithmetic, NUSI_OPT_REFERENCE_ORDER = 1);
        False = the shared-algorithm order (opt-in fast mode, include/nusi.h); True = the reference order explicitly."""
        L = _lib.load()
        self._h = ctypes.c_void_p()
        _lib.check(L.nusi_plan_create(int(device), int(N_bins_E), float(lEmin), float(lEmax), float(zmax),
                                      int(max_points), ctypes.byref(self._h)))
        if reference_order is not None:
            self.set_option(_lib.OPT_REFERENCE_ORDER, 1 if reference_order else 0)
        self.device = device
        self.max_points = max_points
        self.grid_args = (int(N_bins_E), float(lEmin), float(lEmax), float(zmax))
        N, Nz = ctypes.c_int(), ctypes.c_int()
        self.energies = np.zeros(N_bins_E)
        L.nusi_plan_grid(self._h, ctypes.byref(N), ctypes.byref(Nz),
                         self.energies.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        self.N, self.Nz = N.value, Nz.value
        self.T = self.N + self.Nz - 2
        self.PT = self.T * (self.T - 1) // 2

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.load().nusi_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_phiphi(self, alphatilde_path, alpha_path, alphatilde_dims=None, alpha_dims=None):
        d2 = (ctypes.c_int * 2)(*alphatilde_dims) if alphatilde_dims else None
        d3 = (ctypes.c_int * 3)(*alpha_dims) if alpha_dims else None
        _lib.check(_lib.load().nusi_plan_load_phiphi(self._h, alphatilde_path.encode(), d2, alpha_path.encode(), d3))

    def source_axis(self):
        """(lo, hi, z): the bin edges [M = N + Nz - 1] of the source axis -- the energy bins, then the top bin
        redshifted by each step -- and the redshift grid [Nz] (nusi_plan_source_axis)."""
        dp = ctypes.POINTER(ctypes.c_double)
        M = self.T + 1
        lo, hi, z = np.zeros(M), np.zeros(M), np.zeros(self.Nz)
        m = ctypes.c_int()
        _lib.check(_lib.load().nusi_plan_source_axis(self._h, ctypes.byref(m), lo.ctypes.data_as(dp),
                                                     hi.ctypes.data_as(dp), z.ctypes.data_as(dp)))
        assert m.value == M
        return lo, hi, z

    def set_source(self, slot, spectrum, z_weight=None):
        """Register a tabulated source phi(E') W(z) in ``slot``; points select it with
        ``source_model = sources.tabulated(slot)`` (their norm is then absolute, their si ignored).
        spectrum: the bin integrals of dN/dE' over the source axis [M], or a callable dN/dE(E) (integrated per bin,
        sources.bin_integrals); None clears the slot.  z_weight: W(z_i) [Nz] or a callable of z; None = the
        star-formation rate.  Later calls see the new source, earlier results are untouched."""
        from . import sources
        dp = ctypes.POINTER(ctypes.c_double)
        L = _lib.load()
        if spectrum is None:
            _lib.check(L.nusi_plan_set_source(self._h, int(slot), None, None))
            return
        lo, hi, z = self.source_axis()
        S = sources.spectrum_vector(spectrum, lo, hi)
        w = sources.weight_vector(z_weight, z)
        _lib.check(L.nusi_plan_set_source(self._h, int(slot), S.ctypes.data_as(dp),
                                          w.ctypes.data_as(dp) if w is not None else None))

    def params_array(self, points):
        """points: sequence of dicts (calculate_flux keyword arguments) or NusiParams."""
        return params_array(points, self.grid_args)

    def evolve(self, points):
        """Evolve on the GPU; returns host arrays flux, flux_fla of shape (n, 3, N)."""
        arr = points if isinstance(points, ctypes.Array) else self.params_array(points)
        n = len(arr)
        flux = np.zeros((n, 3, self.N))
        fla = np.zeros((n, 3, self.N))
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_evolve_host(self._h, arr, n, flux.ctypes.data_as(dp), fla.ctypes.data_as(dp)))
        return flux, fla

    def evolve_device(self, arr, d_flux_ptr, d_fla_ptr, stream_ptr=None):
        """Asynchronous evolve into device buffers (raw pointers, e.g. torch .data_ptr())."""
        _lib.check(_lib.load().nusi_plan_evolve(self._h, arr, len(arr), ctypes.c_void_p(d_flux_ptr),
                                                ctypes.c_void_p(d_fla_ptr),
                                                ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    # --- response matrices (include/nusi.h "Response matrices") ---
    def _weights(self, z_weight):
        from . import sources
        if z_weight is None:
            return None
        return sources.weight_vector(z_weight, self.source_axis()[2])

    def response(self, points, z_weight=None):
        """The response matrices of the points: host arrays (G, G_fla) of shape (n, M, 3, N), G[p, n, k, b] the flux of
        mass state k in bin b per unit of the source-axis bin integral S[n] (redshift weights z_weight: W(z_i) [Nz],
        a callable of z, or None for the star-formation rate).  The points' si, norm and source_model are ignored, and
        no source slot is read or changed.  flux = norm * sum_n G[p, n] S[n] (response.apply_host, apply_response)."""
        arr = points if isinstance(points, ctypes.Array) else self.params_array(points)
        n, M = len(arr), self.T + 1
        G, Gf = np.zeros((n, M, 3, self.N)), np.zeros((n, M, 3, self.N))
        w = self._weights(z_weight)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_host(self._h, arr, n, w.ctypes.data_as(dp) if w is not None else None,
                                                       G.ctypes.data_as(dp), Gf.ctypes.data_as(dp)))
        return G, Gf

    def response_device(self, arr, d_G_ptr, d_G_fla_ptr, z_weight=None, stream_ptr=None):
        """Asynchronous response into device buffers of n * M * 3 * N doubles (raw pointers; either may be 0 / None)."""
        w = self._weights(z_weight)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response(self._h, arr, len(arr), w.ctypes.data_as(dp) if w is not None else None,
                                                  ctypes.c_void_p(d_G_ptr) if d_G_ptr else None,
                                                  ctypes.c_void_p(d_G_fla_ptr) if d_G_fla_ptr else None,
                                                  ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def _spectra(self, spectra, scale):
        from . import sources
        lo, hi, _ = self.source_axis()
        if callable(spectra) or (isinstance(spectra, np.ndarray) and spectra.ndim == 1):
            spectra = [spectra]
        S = np.ascontiguousarray([sources.spectrum_vector(sp, lo, hi) for sp in spectra], dtype=np.float64)
        sc = None
        if scale is not None:
            sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (len(S),)))
        return S, sc

    def apply_response(self, G, spectra, scale=None):
        """Q spectra on the response matrices G (ntab, M, 3, N) -- G or G_fla of ``response`` -- on the GPU:
        out[t, q] = scale[q] * sum_n G[t, n] S[q, n], shape (ntab, Q, 3, N), bit for bit response.apply_host.
        spectra: a sequence of bin-integral vectors [M] or callables dN/dE(E) (sources.spectrum_vector); scale: None,
        a number or one per spectrum."""
        G = np.ascontiguousarray(G, dtype=np.float64)
        if G.ndim != 4 or G.shape[1:] != (self.T + 1, 3, self.N):
            raise ValueError("apply_response: G must have shape (ntab, %d, 3, %d), got %s" % (self.T + 1, self.N, G.shape))
        S, sc = self._spectra(spectra, scale)
        out = np.zeros((G.shape[0], len(S), 3, self.N))
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_apply_host(self._h, G.ctypes.data_as(dp), G.shape[0], S.ctypes.data_as(dp),
                                                             len(S), sc.ctypes.data_as(dp) if sc is not None else None,
                                                             out.ctypes.data_as(dp)))
        return out

    def apply_response_device(self, d_G_ptr, ntab, spectra, d_out_ptr, scale=None, stream_ptr=None):
        """Asynchronous apply on device-resident response matrices: d_G [ntab][M][3][N], d_out [ntab][Q][3][N] (raw
        pointers); the spectra and scales are host data and are copied.  Returns Q."""
        S, sc = self._spectra(spectra, scale)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_apply(self._h, ctypes.c_void_p(d_G_ptr), int(ntab), S.ctypes.data_as(dp),
                                                        len(S), sc.ctypes.data_as(dp) if sc is not None else None,
                                                        ctypes.c_void_p(d_out_ptr),
                                                        ctypes.c_void_p(stream_ptr) if stream_ptr else None))
        return len(S)

    # --- mass-resolved responses and the source's flavour composition (include/nusi.h "Mass-resolved response") ---
    def step_constants(self):
        """(step_c, step_s): the grid's per-step constants [Nz] (index 0 unused), which response.cascade_host needs."""
        dp = ctypes.POINTER(ctypes.c_double)
        c, s = np.zeros(self.Nz), np.zeros(self.Nz)
        _lib.check(_lib.load().nusi_plan_step_constants(self._h, c.ctypes.data_as(dp), s.ctypes.data_as(dp)))
        return c, s

    def response_mass(self, points, z_weight=None):
        """The response matrices of the points resolved by the source's mass state: host arrays (G3, G3_fla) of shape
        (n, 3, M, 3, N), G3[p, j, n, k, b] the flux of mass state k in bin b per unit of S[n] emitted WHOLLY into mass
        state j.  ``G3.reshape(3 * n, M, 3, N)`` is a stack of ordinary response matrices (apply_response,
        fold_response); ``compose_response`` combines the three of a point into the response of a flavour composition
        (sources.mass_fractions).  Entries with k != j may be slightly negative (include/nusi.h, "Sign")."""
        arr = points if isinstance(points, ctypes.Array) else self.params_array(points)
        n, M = len(arr), self.T + 1
        G, Gf = np.zeros((n, 3, M, 3, self.N)), np.zeros((n, 3, M, 3, self.N))
        w = self._weights(z_weight)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_mass_host(self._h, arr, n, w.ctypes.data_as(dp) if w is not None else None,
                                                            G.ctypes.data_as(dp), Gf.ctypes.data_as(dp)))
        return G, Gf

    def response_mass_device(self, arr, d_G3_ptr, d_G3_fla_ptr, z_weight=None, stream_ptr=None):
        """Asynchronous response_mass into device buffers of n * 3 * M * 3 * N doubles (raw pointers; either may be 0)."""
        w = self._weights(z_weight)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_mass(self._h, arr, len(arr), w.ctypes.data_as(dp) if w is not None else None,
                                                       ctypes.c_void_p(d_G3_ptr) if d_G3_ptr else None,
                                                       ctypes.c_void_p(d_G3_fla_ptr) if d_G3_fla_ptr else None,
                                                       ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    @staticmethod
    def _kappa(kappa, ntab):
        k = np.asarray(kappa, dtype=np.float64)
        if k.ndim == 0 or k.ndim > 3 or k.shape[-1] != 3 or (k.ndim == 3 and k.shape[0] != ntab):
            raise ValueError("compose_response: kappa must have shape (3,), (Qc, 3) or (ntab, Qc, 3), got %s" % (k.shape,))
        if k.ndim == 1:
            k = k[None]
        return np.ascontiguousarray(np.broadcast_to(k, (ntab,) + k.shape[-2:]))

    def compose_response(self, A3, kappa):
        """The composition of mass-resolved rows on the GPU: A3 of shape (ntab, 3, ...) -- G3 / G3_fla of
        ``response_mass``, or a folded stack reshaped to (ntab, 3, M, C) -- and mass fractions kappa of shape (3,),
        (Qc, 3) or (ntab, Qc, 3) (sources.mass_fractions): out[t, c] = (kappa[t, c, 0] A3[t, 0] + kappa[t, c, 1] A3[t, 1])
        + kappa[t, c, 2] A3[t, 2], bit for bit response.compose_host.  Returns (ntab, ...) for a kappa of shape (3,),
        else (ntab, Qc, ...)."""
        A = np.ascontiguousarray(A3, dtype=np.float64)
        if A.ndim < 3 or A.shape[1] != 3:
            raise ValueError("compose_response: A3 must have shape (ntab, 3, ...), got %s" % (A.shape,))
        ntab, rest = A.shape[0], A.shape[2:]
        k = self._kappa(kappa, ntab)
        Qc, X = k.shape[1], int(np.prod(rest))
        out = np.zeros((ntab, Qc) + rest)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_compose_host(self._h, A.ctypes.data_as(dp), ntab, X, k.ctypes.data_as(dp),
                                                               Qc, out.ctypes.data_as(dp)))
        return out[:, 0] if np.ndim(kappa) == 1 else out

    def compose_response_device(self, d_A_ptr, ntab, X, kappa, d_out_ptr, stream_ptr=None):
        """Asynchronous compose on device-resident rows: d_A [ntab][3][X], d_out [ntab][Qc][X] (raw pointers); kappa as
        for compose_response (host data, copied).  Returns Qc."""
        k = self._kappa(kappa, int(ntab))
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_compose(self._h, ctypes.c_void_p(d_A_ptr), int(ntab), int(X),
                                                          k.ctypes.data_as(dp), k.shape[1], ctypes.c_void_p(d_out_ptr),
                                                          ctypes.c_void_p(stream_ptr) if stream_ptr else None))
        return k.shape[1]

    # --- the detector (include/nusi.h "The detector of a plan") ---
    def set_detector(self, D, background=None):
        """Register the detector: D (C, 3, N), D[c, f, b] = expected events in reconstructed bin c per unit of
        flux_fla[f, b] (detector.matrix builds one from bin widths, effective areas, a migration matrix and an exposure),
        and a background expectation per bin (C,), None = 0.  C <= 64; every entry finite and >= 0.  None clears the
        detector.  Later calls see the new detector, earlier results are untouched."""
        dp = ctypes.POINTER(ctypes.c_double)
        L = _lib.load()
        if D is None:
            _lib.check(L.nusi_plan_set_detector(self._h, 0, None, None))
            return
        D = np.ascontiguousarray(D, dtype=np.float64)
        if D.ndim != 3 or D.shape[1:] != (3, self.N):
            raise ValueError("set_detector: D must have shape (C, 3, %d), got %s" % (self.N, D.shape))
        B = None
        if background is not None:
            B = np.ascontiguousarray(np.broadcast_to(np.asarray(background, dtype=np.float64), (D.shape[0],)))
        _lib.check(L.nusi_plan_set_detector(self._h, D.shape[0], D.ctypes.data_as(dp),
                                            B.ctypes.data_as(dp) if B is not None else None))

    def detector_bins(self):
        """C, the detector's reconstructed bins; 0 = no detector."""
        return int(_lib.load().nusi_plan_detector_bins(self._h))

    def fold_flux(self, flux_fla):
        """Expected counts of flavour fluxes (n, 3, N) -- evolve's second output -- on the GPU:
        mu[p, c] = sum_{f, b} flux_fla[p, f, b] D[c, f, b] + background[c], shape (n, C); within gamma_{3N} of exact
        (detector.fold_host; no defined summation order)."""
        F = np.ascontiguousarray(flux_fla, dtype=np.float64)
        if F.ndim != 3 or F.shape[1:] != (3, self.N):
            raise ValueError("fold_flux: flux_fla must have shape (n, 3, %d), got %s" % (self.N, F.shape))
        mu = np.zeros((F.shape[0], self.detector_bins()))
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_fold_flux_host(self._h, F.ctypes.data_as(dp), F.shape[0], mu.ctypes.data_as(dp)))
        return mu

    def fold_flux_device(self, d_flux_fla_ptr, n, d_mu_ptr, stream_ptr=None):
        """Asynchronous fold of device-resident flavour fluxes [n][3][N] into d_mu [n][C] (raw pointers)."""
        _lib.check(_lib.load().nusi_plan_fold_flux(self._h, ctypes.c_void_p(d_flux_fla_ptr), int(n),
                                                   ctypes.c_void_p(d_mu_ptr),
                                                   ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def fold_response(self, G_fla):
        """Fold response matrices G_fla (ntab, M, 3, N) of ``response`` with the detector on the GPU:
        R[t, n, c] = sum_{f, b} G_fla[t, n, f, b] D[c, f, b] (no background), shape (ntab, M, C).  The entries of bins
        b >= n -- exact zeros of a response matrix -- are not read."""
        G = np.ascontiguousarray(G_fla, dtype=np.float64)
        if G.ndim != 4 or G.shape[1:] != (self.T + 1, 3, self.N):
            raise ValueError("fold_response: G_fla must have shape (ntab, %d, 3, %d), got %s" % (self.T + 1, self.N, G.shape))
        R = np.zeros((G.shape[0], self.T + 1, self.detector_bins()))
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_fold_host(self._h, G.ctypes.data_as(dp), G.shape[0], R.ctypes.data_as(dp)))
        return R

    def fold_response_device(self, d_G_fla_ptr, ntab, d_R_ptr, stream_ptr=None):
        """Asynchronous fold of device-resident response matrices [ntab][M][3][N] into d_R [ntab][M][C] (raw pointers)."""
        _lib.check(_lib.load().nusi_plan_response_fold(self._h, ctypes.c_void_p(d_G_fla_ptr), int(ntab),
                                                       ctypes.c_void_p(d_R_ptr),
                                                       ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def _folded(self, R, who):
        """(R as a contiguous (ntab, M, C) array, C) for the call ``who``."""
        R = np.ascontiguousarray(R, dtype=np.float64)
        C = self.detector_bins()
        if C and (R.ndim != 3 or R.shape[1:] != (self.T + 1, C)):   # (no detector: the library refuses, NUSI_ESTATE)
            raise ValueError("%s: R must have shape (ntab, %d, %d), got %s" % (who, self.T + 1, C, R.shape))
        return R, C

    def _data(self, data):
        if data is None:
            return None
        d = np.ascontiguousarray(data, dtype=np.float64)
        if d.shape != (self.detector_bins(),):
            raise ValueError("events: data must have shape (%d,), got %s" % (self.detector_bins(), d.shape))
        return d

    def events(self, R, spectra, scale=None, data=None):
        """Expected counts of Q spectra on folded response matrices R (ntab, M, C) on the GPU:
        mu[t, q, c] = scale[q] * sum_n R[t, n, c] S[q, n] + background[c], shape (ntab, Q, C), bit for bit
        detector.events_host.  With data (C,) also nll[t, q] = sum_c mu - data log mu (detector.poisson_host, the
        Poisson negative log-likelihood without its data-only constant): returns (mu, nll).  spectra and scale as for
        apply_response (scale >= 0 here)."""
        R, C = self._folded(R, "events")
        S, sc = self._spectra(spectra, scale)
        d = self._data(data)
        mu = np.zeros((R.shape[0], len(S), C))
        nll = np.zeros((R.shape[0], len(S))) if d is not None else None
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_events_host(
            self._h, R.ctypes.data_as(dp), R.shape[0], S.ctypes.data_as(dp), len(S),
            sc.ctypes.data_as(dp) if sc is not None else None, d.ctypes.data_as(dp) if d is not None else None,
            mu.ctypes.data_as(dp), nll.ctypes.data_as(dp) if nll is not None else None))
        return mu if d is None else (mu, nll)

    def events_device(self, d_R_ptr, ntab, spectra, d_mu_ptr, d_nll_ptr=None, scale=None, data=None, stream_ptr=None):
        """Asynchronous events on device-resident folded matrices: d_R [ntab][M][C], d_mu [ntab][Q][C] and d_nll
        [ntab][Q] (raw pointers; either output may be 0 / None, d_nll needs data); the spectra, scales and data are
        host data and are copied.  Returns Q."""
        S, sc = self._spectra(spectra, scale)
        d = self._data(data)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_events(
            self._h, ctypes.c_void_p(d_R_ptr), int(ntab), S.ctypes.data_as(dp), len(S),
            sc.ctypes.data_as(dp) if sc is not None else None, d.ctypes.data_as(dp) if d is not None else None,
            ctypes.c_void_p(d_mu_ptr) if d_mu_ptr else None, ctypes.c_void_p(d_nll_ptr) if d_nll_ptr else None,
            ctypes.c_void_p(stream_ptr) if stream_ptr else None))
        return len(S)

    def _minimise(self, who, R, spectra, data, width):
        """profile and fit: (the fitted normalisations (ntab, Q) + width, nll, mu, status) of the library's host form."""
        R, C = self._folded(R, who)
        S, _ = self._spectra(spectra, None)
        d = self._data(data) if C else np.ascontiguousarray(data, dtype=np.float64)     # (no detector: as above)
        ntab, Q = R.shape[0], len(S)
        first, nll, mu = np.zeros((ntab, Q) + width), np.zeros((ntab, Q)), np.zeros((ntab, Q, C))
        status = np.zeros((ntab, Q), dtype=np.int32)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(getattr(_lib.load(), "nusi_plan_response_%s_host" % who)(
            self._h, R.ctypes.data_as(dp), ntab, S.ctypes.data_as(dp), Q, d.ctypes.data_as(dp) if d is not None else None,
            first.ctypes.data_as(dp), nll.ctypes.data_as(dp), mu.ctypes.data_as(dp),
            status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return first, nll, mu, status

    def _minimise_device(self, who, d_R_ptr, ntab, spectra, data, d_first_ptr, d_nll_ptr, d_mu_ptr, d_status_ptr,
                         stream_ptr):
        """profile_device and fit_device: the library's device form on raw pointers.  Returns Q."""
        S, _ = self._spectra(spectra, None)
        d = self._data(data)
        dp = ctypes.POINTER(ctypes.c_double)
        vp = ctypes.c_void_p
        _lib.check(getattr(_lib.load(), "nusi_plan_response_" + who)(
            self._h, vp(d_R_ptr), int(ntab), S.ctypes.data_as(dp), len(S), d.ctypes.data_as(dp) if d is not None else None,
            vp(d_first_ptr) if d_first_ptr else None, vp(d_nll_ptr) if d_nll_ptr else None,
            vp(d_mu_ptr) if d_mu_ptr else None, vp(d_status_ptr) if d_status_ptr else None,
            vp(stream_ptr) if stream_ptr else None))
        return len(S)

    def profile(self, R, spectra, data):
        """The statistic of ``events`` profiled over the flux normalisation, on the GPU: for every table and spectrum
        the a >= 0 that minimises -ln L(a s + background | data), s the expected signal counts of the spectrum at
        scale 1.  Returns (ahat, nll, mu, status): ahat, nll and status of shape (ntab, Q), mu = ahat s + background of
        shape (ntab, Q, C); status holds the Newton steps taken in its low 8 bits and the _lib.FIT_* flags above
        (FIT_FLAT: no signal or no data in any signal bin, ahat = 0; FIT_BOUNDARY: the minimum is at a = 0;
        FIT_NOT_CONVERGED; FIT_INFINITE: a bin with data has neither signal nor background, nll = +inf).  ahat, mu and
        status equal detector.profile_host bit for bit.  There is no scale: it is what is fitted."""
        return self._minimise("profile", R, spectra, data, ())

    def profile_device(self, d_R_ptr, ntab, spectra, data, d_ahat_ptr, d_nll_ptr=None, d_mu_ptr=None, d_status_ptr=None,
                       stream_ptr=None):
        """Asynchronous profile on device-resident folded matrices: d_R [ntab][M][C], d_ahat and d_nll [ntab][Q],
        d_mu [ntab][Q][C] (doubles) and d_status [ntab][Q] (ints) are raw pointers, every output but d_ahat may be
        0 / None; the spectra and data are host data and are copied.  Returns Q."""
        return self._minimise_device("profile", d_R_ptr, ntab, spectra, data, d_ahat_ptr, d_nll_ptr, d_mu_ptr,
                                     d_status_ptr, stream_ptr)

    def set_templates(self, templates, prior=None):
        """Register K <= 3 background templates (K, C) of the detector -- expected counts per reconstructed bin at
        normalisation 1, entries finite and >= 0, none all zeros -- whose normalisations ``fit`` floats with the
        signal's.  prior: None or (mean (K,), sigma (K,)), a Gaussian constraint per template (mean >= 0, sigma > 0,
        sigma = inf: none).  None clears the templates; so does set_detector."""
        dp = ctypes.POINTER(ctypes.c_double)
        L = _lib.load()
        if templates is None:
            _lib.check(L.nusi_plan_set_templates(self._h, 0, None, None, None))
            return
        T = np.ascontiguousarray(templates, dtype=np.float64)
        if T.ndim == 1:
            T = T[None]
        C = self.detector_bins()
        if C and (T.ndim != 2 or T.shape[1] != C):           # (no detector: the library refuses, NUSI_ESTATE)
            raise ValueError("set_templates: templates must have shape (K, %d), got %s" % (C, T.shape))
        K = T.shape[0]
        mean = sigma = None
        if prior is not None:
            mean, sigma = prior
            if mean is not None:
                mean = np.ascontiguousarray(np.broadcast_to(np.asarray(mean, dtype=np.float64), (K,)))
            if sigma is not None:
                sigma = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (K,)))
        _lib.check(L.nusi_plan_set_templates(self._h, K, T.ctypes.data_as(dp),
                                             mean.ctypes.data_as(dp) if mean is not None else None,
                                             sigma.ctypes.data_as(dp) if sigma is not None else None))

    def templates(self):
        """K, the number of background templates; 0 = none."""
        return int(_lib.load().nusi_plan_templates(self._h))

    def fit(self, R, spectra, data):
        """The statistic of ``events`` minimised over the signal's scale and the templates' normalisations at once, on
        the GPU: theta >= 0 minimising sum_c (mu_c - data_c log mu_c) + sum_j (theta_j - mean_j)^2 / (2 sigma_j^2),
        mu = theta_0 s + sum_j theta_j T_j + background.  Returns (theta (ntab, Q, 1 + K), nll (ntab, Q),
        mu (ntab, Q, C), status (ntab, Q) int32): the Newton steps in the low 8 bits, the _lib.FIT_* flags (FIT_FLAT:
        no signal, the templates are still fitted; FIT_BOUNDARY: theta_0 = 0; FIT_NOT_CONVERGED; FIT_SINGULAR: the
        data do not determine the components; FIT_INFINITE), FIT_ZERO << j for a component that ends at zero and the
        halvings from bit FIT_TRIALS_SHIFT.  theta, mu and status equal detector.fit_host bit for bit."""
        return self._minimise("fit", R, spectra, data, (1 + self.templates(),))

    def fit_device(self, d_R_ptr, ntab, spectra, data, d_theta_ptr, d_nll_ptr=None, d_mu_ptr=None, d_status_ptr=None,
                   stream_ptr=None):
        """Asynchronous fit on device-resident folded matrices: d_R [ntab][M][C], d_theta [ntab][Q][1 + K], d_nll
        [ntab][Q], d_mu [ntab][Q][C] (doubles) and d_status [ntab][Q] (ints) are raw pointers, every output but
        d_theta may be 0 / None; the spectra and data are host data and are copied.  Returns Q."""
        return self._minimise_device("fit", d_R_ptr, ntab, spectra, data, d_theta_ptr, d_nll_ptr, d_mu_ptr, d_status_ptr,
                                     stream_ptr)

    def _stack(self, R3, who):
        """(R3 as a contiguous (ntab, J, M, C) array, J, C) for the call ``who``."""
        R3 = np.ascontiguousarray(R3, dtype=np.float64)
        C = self.detector_bins()
        if R3.ndim != 4 or (C and R3.shape[2:] != (self.T + 1, C)):   # (no detector: the library refuses, NUSI_ESTATE)
            raise ValueError("%s: R3 must have shape (ntab, J, %d, %d), got %s" % (who, self.T + 1, C, R3.shape))
        return R3, R3.shape[1], C

    def fit_components(self, R3, spectra, data):
        """``fit`` with J = 2 .. 3 SIGNAL components per table and spectrum, on the GPU: R3 (ntab, J, M, C) is a stack
        of folded matrices -- the folded rows of ``response_mass``, or those rows composed onto the pure flavours
        (``compose_response`` with sources.mass_fractions of e, mu, tau) -- and every normalisation floats, >= 0, together
        with the plan's K = 0 .. 3 templates: mu = sum_j theta_j s_j + sum_i theta_{J+i-1} T_i + background.  Returns
        (theta (ntab, Q, J + K), nll (ntab, Q), mu (ntab, Q, C), status (ntab, Q) int32) as ``fit`` does; FIT_FLAT: no
        signal component is live (the templates are fitted all the same), FIT_BOUNDARY: every signal theta_j ends at 0,
        FIT_ZERO << j for j < J + K, FIT_SINGULAR: the data do not tell the components apart (proportional rows, or
        fewer bins with data than components).  theta, mu and status equal detector.fit_components_host bit for bit;
        detector.composition(theta, J) gives the total and the fitted shares.  J = 1 is ``fit`` / ``profile``."""
        R3, J, C = self._stack(R3, "fit_components")
        S, _ = self._spectra(spectra, None)
        d = self._data(data) if C else np.ascontiguousarray(data, dtype=np.float64)     # (no detector: as above)
        ntab, Q = R3.shape[0], len(S)
        theta, nll, mu = np.zeros((ntab, Q, J + self.templates())), np.zeros((ntab, Q)), np.zeros((ntab, Q, C))
        status = np.zeros((ntab, Q), dtype=np.int32)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_fit_components_host(
            self._h, R3.ctypes.data_as(dp), ntab, J, S.ctypes.data_as(dp), Q, d.ctypes.data_as(dp) if d is not None else None,
            theta.ctypes.data_as(dp), nll.ctypes.data_as(dp), mu.ctypes.data_as(dp),
            status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return theta, nll, mu, status

    def fit_components_device(self, d_R3_ptr, ntab, J, spectra, data, d_theta_ptr, d_nll_ptr=None, d_mu_ptr=None,
                              d_status_ptr=None, stream_ptr=None):
        """Asynchronous fit_components on a device-resident stack: d_R3 [ntab][J][M][C], d_theta [ntab][Q][J + K], d_nll
        [ntab][Q], d_mu [ntab][Q][C] (doubles) and d_status [ntab][Q] (ints) are raw pointers, every output but d_theta
        may be 0 / None; the spectra and data are host data and are copied.  Returns Q."""
        S, _ = self._spectra(spectra, None)
        d = self._data(data)
        dp = ctypes.POINTER(ctypes.c_double)
        vp = ctypes.c_void_p
        _lib.check(_lib.load().nusi_plan_response_fit_components(
            self._h, vp(d_R3_ptr), int(ntab), int(J), S.ctypes.data_as(dp), len(S),
            d.ctypes.data_as(dp) if d is not None else None, vp(d_theta_ptr) if d_theta_ptr else None,
            vp(d_nll_ptr) if d_nll_ptr else None, vp(d_mu_ptr) if d_mu_ptr else None,
            vp(d_status_ptr) if d_status_ptr else None, vp(stream_ptr) if stream_ptr else None))
        return len(S)

    def composition_scan(self, R3, spectra, data, phi, prior=None):
        """The statistic q(phi) = 2 (min f at the composition phi - the free minimum) that draws a contour in the flavour
        triangle.  R3 (ntab, 3, M, C): three folded rows per table; phi (Qc, 3) or (ntab, Qc, 3): weights >= 0 on those
        rows.  It composes R = compose_response(R3, phi), fits every composed matrix with the scale floating -- ``profile``
        without templates, ``fit`` with them -- fits the components freely with ``fit_components`` on R3, and forms
        lambda with detector.composition_statistic.  prior: the (mean, sigma) given to set_templates (the plan does not
        hand them back), None = no penalty terms.

        The free fit spans a_j >= 0 on the GIVEN rows: on raw mass-resolved rows that is the cone of mass fractions >= 0,
        which is larger than what any flavour composition reaches.  To restrict it to the physical flavour triangle, pass
        rows composed onto the pure flavours, R3 = compose_response(R3_mass, [mass_fractions(e_f) for f in e, mu, tau]),
        with phi then the flavour fractions themselves.

        Returns (q (ntab, Qc, Q) = max(2 lambda, 0), fixed, free, word): fixed = (theta (ntab, Qc, Q, 1 + K), nll, mu,
        status) of the fits at the held compositions, free = fit_components' four arrays, word (ntab, Qc, Q) int32 = the
        FIT_NOT_CONVERGED, FIT_SINGULAR and FIT_INFINITE flags of either fit, ORed per entry (0: q is a statistic)."""
        from . import detector as _det
        R3, J, C = self._stack(R3, "composition_scan")
        if J != 3:
            raise ValueError("composition_scan: R3 must have shape (ntab, 3, M, C), got %s" % (R3.shape,))
        ntab, M = R3.shape[0], R3.shape[2]
        k = self._kappa(phi, ntab)
        if np.ndim(phi) == 1:
            raise ValueError("composition_scan: phi must have shape (Qc, 3) or (ntab, Qc, 3)")
        Qc, K = k.shape[1], self.templates()
        R = self.compose_response(R3, k).reshape(ntab * Qc, M, C)
        if K:
            th, nll, mu, st = self.fit(R, spectra, data)
        else:
            ah, nll, mu, st = self.profile(R, spectra, data)
            th = ah[..., None]
        Q = nll.shape[1]
        fixed = (th.reshape(ntab, Qc, Q, 1 + K), nll.reshape(ntab, Qc, Q), mu.reshape(ntab, Qc, Q, C),
                 st.reshape(ntab, Qc, Q))
        free = self.fit_components(R3, spectra, data)
        lam, _ = _det.composition_statistic(fixed[2], fixed[0], free[2][:, None], free[0][:, None],
                                            np.asarray(data, dtype=np.float64), prior=prior, log=np.log)
        with np.errstate(invalid="ignore"):
            q = np.where(np.isnan(lam), np.nan, np.maximum(2.0 * lam, 0.0))
        bad = _lib.FIT_NOT_CONVERGED | _lib.FIT_SINGULAR | _lib.FIT_INFINITE
        word = ((fixed[3] & bad) | (free[3][:, None] & bad)).astype(np.int32)
        return q, fixed, free, word

    def _held(self, who, scale, Q):
        if scale is None:
            raise ValueError("%s: the held scale is required (a number or (Q,))" % who)
        return np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (Q,)))

    def fit_fixed(self, R, spectra, scale, data):
        """The conditional fit on the GPU: ``fit`` with the signal's scale HELD at ``scale`` (a number, or (Q,) one per
        spectrum, >= 0) and only the templates' normalisations floating -- the background-only fit at scale 0, and
        the inner minimum of the statistic q(a) = 2 (min_theta f(a, theta) - min f) at any a.  Returns (theta
        (ntab, Q, 1 + K) with theta[..., 0] = scale, nll (ntab, Q), mu (ntab, Q, C), status (ntab, Q) int32) as ``fit``
        does; the status word holds the steps, FIT_NOT_CONVERGED, FIT_SINGULAR, FIT_INFINITE, FIT_ZERO << j for a
        template that ends at zero and the halvings -- never FIT_FLAT, FIT_BOUNDARY or FIT_ZERO << 0.  theta, mu and
        status equal detector.fit_fixed_host bit for bit, and mu has the bits ``fit``'s mu has at the same theta."""
        R, C = self._folded(R, "fit_fixed")
        S, _ = self._spectra(spectra, None)
        sc = self._held("fit_fixed", scale, len(S))
        d = self._data(data) if C else np.ascontiguousarray(data, dtype=np.float64)     # (no detector: as above)
        ntab, Q = R.shape[0], len(S)
        theta, nll, mu = np.zeros((ntab, Q, 1 + self.templates())), np.zeros((ntab, Q)), np.zeros((ntab, Q, C))
        status = np.zeros((ntab, Q), dtype=np.int32)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_fit_fixed_host(
            self._h, R.ctypes.data_as(dp), ntab, S.ctypes.data_as(dp), Q, sc.ctypes.data_as(dp),
            d.ctypes.data_as(dp) if d is not None else None, theta.ctypes.data_as(dp), nll.ctypes.data_as(dp),
            mu.ctypes.data_as(dp), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return theta, nll, mu, status

    def fit_fixed_device(self, d_R_ptr, ntab, spectra, scale, data, d_theta_ptr, d_nll_ptr=None, d_mu_ptr=None,
                         d_status_ptr=None, stream_ptr=None):
        """Asynchronous conditional fit on device-resident folded matrices: the pointers as for ``fit_device``; the
        spectra, the held scales and the data are host data and are copied.  Returns Q."""
        S, _ = self._spectra(spectra, None)
        sc = self._held("fit_fixed_device", scale, len(S))
        d = self._data(data)
        dp = ctypes.POINTER(ctypes.c_double)
        vp = ctypes.c_void_p
        _lib.check(_lib.load().nusi_plan_response_fit_fixed(
            self._h, vp(d_R_ptr), int(ntab), S.ctypes.data_as(dp), len(S), sc.ctypes.data_as(dp),
            d.ctypes.data_as(dp) if d is not None else None, vp(d_theta_ptr) if d_theta_ptr else None,
            vp(d_nll_ptr) if d_nll_ptr else None, vp(d_mu_ptr) if d_mu_ptr else None,
            vp(d_status_ptr) if d_status_ptr else None, vp(stream_ptr) if stream_ptr else None))
        return len(S)

    @staticmethod
    def _which(which):
        w = {"lower": _lib.LIMIT_LOWER, "upper": _lib.LIMIT_UPPER, "both": _lib.LIMIT_LOWER | _lib.LIMIT_UPPER}.get(which, which)
        return int(w)

    def limit(self, R, spectra, data, delta, which="upper"):
        """Profile-likelihood limits on the signal's scale on the GPU: for every table and spectrum the best fit
        (``fit``'s record; ``profile``'s on a plan without templates) and the roots a_lo < theta_hat_0 < a_hi of
        q(a) = 2 (min_theta f(a, theta) - min f) = delta -- delta = 2.706 for a one-sided 95 % upper limit, 1 for a 68 %
        interval -- found inside one kernel: the signal counts are computed once, and the search costs only its own
        arithmetic.  which: "upper", "lower" or "both".  Returns (lo (ntab, Q), hi (ntab, Q), theta_hat (ntab, Q, 1 + K),
        nll_hat (ntab, Q), status (ntab, Q, 3) int32): the best fit's word (bit for bit ``fit``'s or ``profile``'s, like
        theta_hat and nll_hat), then the lower and the upper side's: the outer steps in the low 8 bits, _lib.LIMIT_AT_ZERO
        (a_lo = 0: the statistic at zero is within delta), LIMIT_UNBOUNDED (no signal counts: a_hi = +inf),
        LIMIT_NO_FIT (the best fit failed: NaN), LIMIT_NOT_CONVERGED, and the inner Newton steps from bit
        LIMIT_INNER_SHIFT.  A side not asked for is NaN with a word of 0.  detector.limit_host is the same search in
        numpy."""
        R, C = self._folded(R, "limit")
        S, _ = self._spectra(spectra, None)
        d = self._data(data) if C else np.ascontiguousarray(data, dtype=np.float64)     # (no detector: as above)
        ntab, Q = R.shape[0], len(S)
        lo, hi = np.full((ntab, Q), np.nan), np.full((ntab, Q), np.nan)
        theta, nll = np.zeros((ntab, Q, 1 + self.templates())), np.zeros((ntab, Q))
        status = np.zeros((ntab, Q, 3), dtype=np.int32)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_response_limit_host(
            self._h, R.ctypes.data_as(dp), ntab, S.ctypes.data_as(dp), Q, d.ctypes.data_as(dp) if d is not None else None,
            float(delta), self._which(which), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), theta.ctypes.data_as(dp),
            nll.ctypes.data_as(dp), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return lo, hi, theta, nll, status

    def limit_device(self, d_R_ptr, ntab, spectra, data, delta, which, d_lo_ptr, d_hi_ptr, d_theta_hat_ptr=None,
                     d_nll_hat_ptr=None, d_status_ptr=None, stream_ptr=None):
        """Asynchronous limits on device-resident folded matrices: d_R [ntab][M][C], d_lo, d_hi and d_nll_hat [ntab][Q],
        d_theta_hat [ntab][Q][1 + K] (doubles) and d_status [ntab][Q][3] (ints) are raw pointers; any may be 0 / None
        but the result of a side asked for; the spectra and data are host data and are copied.  Returns Q."""
        S, _ = self._spectra(spectra, None)
        d = self._data(data)
        dp = ctypes.POINTER(ctypes.c_double)
        vp = ctypes.c_void_p
        _lib.check(_lib.load().nusi_plan_response_limit(
            self._h, vp(d_R_ptr), int(ntab), S.ctypes.data_as(dp), len(S), d.ctypes.data_as(dp) if d is not None else None,
            float(delta), self._which(which), vp(d_lo_ptr) if d_lo_ptr else None, vp(d_hi_ptr) if d_hi_ptr else None,
            vp(d_theta_hat_ptr) if d_theta_hat_ptr else None, vp(d_nll_hat_ptr) if d_nll_hat_ptr else None,
            vp(d_status_ptr) if d_status_ptr else None, vp(stream_ptr) if stream_ptr else None))
        return len(S)

    def _datasets(self, datasets):
        d = np.ascontiguousarray(datasets, dtype=np.float64)
        if d.ndim == 1:
            d = d[None]
        C = self.detector_bins()
        if C and (d.ndim != 2 or d.shape[0] < 1 or d.shape[1] != C):   # (no detector: the library refuses, NUSI_ESTATE)
            raise ValueError("ensemble: datasets must have shape (P, %d), P >= 1, got %s" % (C, d.shape))
        return d

    def ensemble(self, R, spectra, datasets):
        """P data sets -- an ensemble of pseudo-experiments, datasets (P, C) -- against every table and spectrum in one
        call on the GPU, and of each (p, t) only the best spectrum's record: the signal counts of (t, q) are computed
        once and the P fits run on them.  The record of a spectrum is what ``fit`` gives for it against datasets[p]
        (``profile`` on a plan without templates, K = 0: theta is ahat), bit for bit; the best is the minimum under the
        key (isnan(nll), nll, q) -- detector.argbest: a NaN loses to everything, ties go to the lowest q.  Returns
        (q (P, ntab) int32, nll (P, ntab), theta (P, ntab, 1 + K), status (P, ntab) int32), the same as
        detector.ensemble_host up to the last bits of nll's log.  This call draws no random numbers: the toys are host
        data (detector.pseudo_data, or ``draw``)."""
        R, C = self._folded(R, "ensemble")
        S, _ = self._spectra(spectra, None)
        d = self._datasets(datasets)
        ntab, P, W = R.shape[0], d.shape[0], 1 + self.templates()
        q, status = np.zeros((P, ntab), dtype=np.int32), np.zeros((P, ntab), dtype=np.int32)
        nll, theta = np.zeros((P, ntab)), np.zeros((P, ntab, W))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        _lib.check(_lib.load().nusi_plan_response_ensemble_host(
            self._h, R.ctypes.data_as(dp), ntab, S.ctypes.data_as(dp), len(S), d.ctypes.data_as(dp), P,
            q.ctypes.data_as(ip), nll.ctypes.data_as(dp), theta.ctypes.data_as(dp), status.ctypes.data_as(ip)))
        return q, nll, theta, status

    def ensemble_device(self, d_R_ptr, ntab, spectra, datasets, d_q_ptr, d_nll_ptr, d_theta_ptr=None, d_status_ptr=None,
                        stream_ptr=None):
        """Asynchronous ensemble on device-resident folded matrices: d_R [ntab][M][C], d_q and d_status [P][ntab]
        (ints), d_nll [P][ntab] and d_theta [P][ntab][1 + K] (doubles) are raw pointers, d_theta and d_status may be
        0 / None; the spectra and the data sets are host data and are copied.  Returns (Q, P)."""
        S, _ = self._spectra(spectra, None)
        d = self._datasets(datasets) if datasets is not None else None
        dp = ctypes.POINTER(ctypes.c_double)
        vp = ctypes.c_void_p
        _lib.check(_lib.load().nusi_plan_response_ensemble(
            self._h, vp(d_R_ptr), int(ntab), S.ctypes.data_as(dp), len(S), d.ctypes.data_as(dp) if d is not None else None,
            d.shape[0] if d is not None else 0, vp(d_q_ptr) if d_q_ptr else None, vp(d_nll_ptr) if d_nll_ptr else None,
            vp(d_theta_ptr) if d_theta_ptr else None, vp(d_status_ptr) if d_status_ptr else None,
            vp(stream_ptr) if stream_ptr else None))
        return len(S), (d.shape[0] if d is not None else 0)

    def _ranks(self, ranks, P):
        from . import detector
        r = detector.band_ranks(P) if ranks is None else np.asarray(ranks, dtype=np.int64).reshape(-1)
        return np.ascontiguousarray(r, dtype=np.int32)

    def ensemble_limit(self, R, spectra, datasets, delta, which="upper", ranks=None, raw=False):
        """The limits of ``limit`` for P data sets -- datasets (P, C), an ensemble of pseudo-experiments -- in one call on
        the GPU, and per table and spectrum the order statistics of its P limits: with background-only toys the median
        expected limit and its bands.  The signal counts of (t, q) are computed once and the P searches run on them; the
        record of (p, t, q) is what ``limit`` gives against datasets[p], bit for bit.  ranks: ints in 0 .. P - 1, at most
        _lib.BAND_RANKS_MAX of them (None: detector.band_ranks(P), the 2.5, 16, 50, 84 and 97.5 % points); the band is
        detector.order_stat of the P limits -- a NaN (no fit) sorts after +inf (no signal).  Returns (band_lo (ntab, Q,
        NR), band_hi (ntab, Q, NR), tally (ntab, Q, 2, 4) int32): per side (0 lower, 1 upper) the toys flagged
        _lib.LIMIT_AT_ZERO, LIMIT_UNBOUNDED, LIMIT_NO_FIT and LIMIT_NOT_CONVERGED; with raw also (lo_all (ntab, Q, P),
        hi_all (ntab, Q, P), words_all (ntab, Q, P, 2) int32), every toy's limits and side words.  A side not asked for
        has NaN bands, a tally of 0 and words of 0.  detector.ensemble_limit_host is the same in numpy."""
        R, C = self._folded(R, "ensemble_limit")
        S, _ = self._spectra(spectra, None)
        d = self._datasets(datasets)
        ntab, Q, P = R.shape[0], len(S), d.shape[0]
        r = self._ranks(ranks, P)
        NR = len(r)
        band_lo, band_hi = np.full((ntab, Q, NR), np.nan), np.full((ntab, Q, NR), np.nan)
        tally = np.zeros((ntab, Q, 2, 4), dtype=np.int32)
        lo_all = hi_all = words = None
        if raw:
            lo_all, hi_all = np.full((ntab, Q, P), np.nan), np.full((ntab, Q, P), np.nan)
            words = np.zeros((ntab, Q, P, 2), dtype=np.int32)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        _lib.check(_lib.load().nusi_plan_response_ensemble_limit_host(
            self._h, R.ctypes.data_as(dp), ntab, S.ctypes.data_as(dp), Q, d.ctypes.data_as(dp), P, float(delta),
            self._which(which), r.ctypes.data_as(ip), NR, band_lo.ctypes.data_as(dp), band_hi.ctypes.data_as(dp),
            tally.ctypes.data_as(ip), lo_all.ctypes.data_as(dp) if raw else None, hi_all.ctypes.data_as(dp) if raw else None,
            words.ctypes.data_as(ip) if raw else None))
        return (band_lo, band_hi, tally) + ((lo_all, hi_all, words) if raw else ())

    def ensemble_limit_device(self, d_R_ptr, ntab, spectra, datasets, delta, which, ranks, d_band_lo_ptr, d_band_hi_ptr,
                              d_tally_ptr=None, d_lo_all_ptr=None, d_hi_all_ptr=None, d_words_all_ptr=None, stream_ptr=None):
        """Asynchronous ensemble_limit on device-resident folded matrices: d_R [ntab][M][C], d_band_lo and d_band_hi
        [ntab][Q][NR], d_lo_all and d_hi_all [ntab][Q][P] (doubles), d_tally [ntab][Q][2][4] and d_words_all
        [ntab][Q][P][2] (ints) are raw pointers; any may be 0 / None, but with ranks the band of a side asked for is
        needed.  ranks: ints (None: detector.band_ranks(P); an empty list: no band).  The spectra, the data sets and
        the ranks are host data and are copied.  Returns (Q, P, NR)."""
        S, _ = self._spectra(spectra, None)
        d = self._datasets(datasets) if datasets is not None else None
        P = d.shape[0] if d is not None else 0
        r = self._ranks(ranks, max(P, 1))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        vp = ctypes.c_void_p
        _lib.check(_lib.load().nusi_plan_response_ensemble_limit(
            self._h, vp(d_R_ptr), int(ntab), S.ctypes.data_as(dp), len(S), d.ctypes.data_as(dp) if d is not None else None, P,
            float(delta), self._which(which), r.ctypes.data_as(ip) if len(r) else None, len(r),
            vp(d_band_lo_ptr) if d_band_lo_ptr else None, vp(d_band_hi_ptr) if d_band_hi_ptr else None,
            vp(d_tally_ptr) if d_tally_ptr else None, vp(d_lo_all_ptr) if d_lo_all_ptr else None,
            vp(d_hi_all_ptr) if d_hi_all_ptr else None, vp(d_words_all_ptr) if d_words_all_ptr else None,
            vp(stream_ptr) if stream_ptr else None))
        return len(S), P, len(r)

    # --- the generator (include/nusi.h "Drawing counts") ---
    @staticmethod
    def _expectations(mu):
        m = np.ascontiguousarray(mu, dtype=np.float64)
        one = m.ndim == 1
        if one:
            m = m[None]
        if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
            raise ValueError("draw: mu must have shape (C,) or (rows, C), got %s" % (np.shape(mu),))
        return m, one

    def draw(self, mu, P, seed, stream=0):
        """P Poisson pseudo-experiments around the expected counts mu (rows, C) or (C,), drawn on the GPU by the
        counter-based generator include/nusi.h defines: counts (rows, P, C), or (P, C) for a vector, as float64.  The
        count of (row, p, c) depends on (seed, stream, row, p, c) alone -- seed a 64-bit, stream a 32-bit unsigned
        int -- and is detector.draw_host's, every integer.  No detector is needed; C <= 64, mu finite and >= 0."""
        m, one = self._expectations(mu)
        out = np.zeros((m.shape[0], int(P), m.shape[1]))
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_draw_counts_host(self._h, m.ctypes.data_as(dp), m.shape[0], m.shape[1], int(P),
                                                          int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 32 - 1),
                                                          out.ctypes.data_as(dp)))
        return out[0] if one else out

    def draw_device(self, mu, P, seed, d_out_ptr, stream=0, stream_ptr=None):
        """Asynchronous ``draw`` into device memory: d_out [rows][P][C] doubles (a raw pointer); mu is host data and is
        copied.  Returns (rows, C)."""
        m, _ = self._expectations(mu)
        dp = ctypes.POINTER(ctypes.c_double)
        vp = ctypes.c_void_p
        _lib.check(_lib.load().nusi_plan_draw_counts(self._h, m.ctypes.data_as(dp), m.shape[0], m.shape[1], int(P),
                                                     int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 32 - 1),
                                                     vp(d_out_ptr) if d_out_ptr else None,
                                                     vp(stream_ptr) if stream_ptr else None))
        return m.shape

    @staticmethod
    def _normal_args(center, sigma):
        c = np.ascontiguousarray(center, dtype=np.float64)
        one = c.ndim == 1
        if one:
            c = c[None]
        if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1:
            raise ValueError("draw_normal: center must have shape (J,) or (rows, J), got %s" % (np.shape(center),))
        sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (c.shape[1],)))
        return c, sg, one

    def draw_normal(self, center, sigma, P, seed, stream=0):
        """P normal variates around every center (rows, J) or (J,), of the widths sigma (J,) or a number, truncated to
        x >= 0, drawn on the GPU by the generator include/nusi.h defines ("Drawing normals"): float64 (rows, P, J), or
        (P, J) for a vector.  The variate of (row, p, j) depends on (seed, stream, row, p, j) alone and is
        detector.draw_normal_host's, every bit; its Philox blocks are none of ``draw``'s.  center finite and >= 0, sigma
        > 0 (inf: the center itself, no bits drawn), J <= 64.  No detector is needed."""
        c, sg, one = self._normal_args(center, sigma)
        out = np.zeros((c.shape[0], int(P), c.shape[1]))
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_draw_normals_host(self._h, c.ctypes.data_as(dp), sg.ctypes.data_as(dp), c.shape[0],
                                                           c.shape[1], int(P), int(seed) & (2 ** 64 - 1),
                                                           int(stream) & (2 ** 32 - 1), out.ctypes.data_as(dp)))
        return out[0] if one else out

    def draw_normal_device(self, center, sigma, P, seed, d_out_ptr, stream=0, stream_ptr=None):
        """Asynchronous ``draw_normal`` into device memory: d_out [rows][P][J] doubles (a raw pointer); center and sigma
        are host data and are copied.  Returns (rows, J)."""
        c, sg, _ = self._normal_args(center, sigma)
        dp = ctypes.POINTER(ctypes.c_double)
        vp = ctypes.c_void_p
        _lib.check(_lib.load().nusi_plan_draw_normals(self._h, c.ctypes.data_as(dp), sg.ctypes.data_as(dp), c.shape[0],
                                                      c.shape[1], int(P), int(seed) & (2 ** 64 - 1),
                                                      int(stream) & (2 ** 32 - 1), vp(d_out_ptr) if d_out_ptr else None,
                                                      vp(stream_ptr) if stream_ptr else None))
        return c.shape

    # --- the calibration call (include/nusi.h nusi_plan_response_inject) ---
    def _nuisance(self, nuisance):
        """nuisance: None leaves the plan's NUSI_OPT_TOY_NUISANCE alone; "fixed", "global", "prior" or _lib.TOYS_* sets it."""
        if nuisance is not None:
            self.set_option(_lib.OPT_TOY_NUISANCE, int({"fixed": _lib.TOYS_FIXED, "global": _lib.TOYS_GLOBAL,
                                                        "prior": _lib.TOYS_PRIOR}.get(nuisance, nuisance)))

    @staticmethod
    def _mode(mode):
        return int({"two-sided": _lib.INJECT_TWO_SIDED, "upper": _lib.INJECT_UPPER,
                    "discovery": _lib.INJECT_DISCOVERY}.get(mode, mode))

    def _inject_args(self, spectra, a_inj, theta_inj, a_test, ranks, P, q_obs, ntab):
        S, _ = self._spectra(spectra, None)
        Q = len(S)
        ai = self._held("inject", a_inj, Q)
        at = None if a_test is None else self._held("inject", a_test, Q)
        ti = None
        if theta_inj is not None:
            ti = np.ascontiguousarray(np.broadcast_to(np.asarray(theta_inj, dtype=np.float64), (self.templates(),)))
        qo = None
        if q_obs is not None:
            qo = np.ascontiguousarray(np.broadcast_to(np.asarray(q_obs, dtype=np.float64), (ntab, Q)))
        return S, ai, ti, at, self._ranks(ranks, max(int(P), 1)), qo

    def inject(self, R, spectra, a_inj, P, seed, theta_inj=None, a_test=None, mode="two-sided", ranks=None, q_obs=None,
               raw=False, nuisance=None):
        """The distribution of the statistic q(a_test) on toys drawn from a hypothesis's own expectation, in one call on
        the GPU.  For every table t, spectrum q and toy p < P the counts are drawn on the device from
        a_inj[q] s + sum_j theta_inj[j] T_j + B -- ``draw`` of that expectation with stream = t at [q, p] --, fitted
        (``fit``'s record; ``profile``'s without templates), fitted again with the signal held at a_test[q] (None: a_inj;
        ``fit_fixed``'s record from its cold start) and stat = max(2 lambda, 0) is formed as ``limit`` forms lambda.  mode:
        "two-sided", "upper" (stat = 0 where theta_hat_0 > a_test) or "discovery" (stat = 0 where theta_hat_0 < a_test).
        a_inj, a_test: a number or (Q,); theta_inj: (K,), None = the templates' prior means; ranks: None =
        detector.band_ranks(P); q_obs: None, a number or (ntab, Q).  Returns (band_theta (ntab, Q, NR), band_stat (ntab,
        Q, NR), tally (ntab, Q, 4) int32) -- the order statistics of theta_hat_0 and of stat over the toys, NaN (a failed
        fit) last, and the toys whose best fit failed, whose conditional fit alone failed, with theta_hat_0 = 0 and with an
        infinite best fit --, with q_obs also exceed (ntab, Q) int32, the toys with stat >= q_obs (the p-value:
        exceed / (P - tally[..., 0] - tally[..., 1])), and with raw also (theta_all (ntab, Q, P), stat_all (ntab, Q, P),
        words_all (ntab, Q, P, 2) int32, data_all (ntab, Q, P, C)).  detector.inject_host is the same in numpy.

        nuisance: the toys' ensemble for templates under a prior -- "fixed" (the prior means stay), "global" (the means,
        as auxiliary measurements, are redrawn per toy around theta_inj: ``draw_normal`` with stream = t at [q, p, j]) or
        "prior" (the nuisances themselves are drawn around the prior means and the counts follow them;
        Cousins-Highland), or _lib.TOYS_*; it sets the plan's OPT_TOY_NUISANCE, None leaves it alone."""
        self._nuisance(nuisance)
        R, C = self._folded(R, "inject")
        ntab, P = R.shape[0], int(P)
        S, ai, ti, at, r, qo = self._inject_args(spectra, a_inj, theta_inj, a_test, ranks, P, q_obs, ntab)
        Q, NR = len(S), len(r)
        band_th, band_st = np.full((ntab, Q, NR), np.nan), np.full((ntab, Q, NR), np.nan)
        tally = np.zeros((ntab, Q, 4), dtype=np.int32)
        exceed = np.zeros((ntab, Q), dtype=np.int32) if qo is not None else None
        th_all = st_all = words = data = None
        if raw:
            th_all, st_all = np.full((ntab, Q, max(P, 0)), np.nan), np.full((ntab, Q, max(P, 0)), np.nan)
            words, data = np.zeros((ntab, Q, max(P, 0), 2), dtype=np.int32), np.zeros((ntab, Q, max(P, 0), C))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)

        def ptr(x, t):
            return x.ctypes.data_as(t) if x is not None else None
        _lib.check(_lib.load().nusi_plan_response_inject_host(
            self._h, R.ctypes.data_as(dp), ntab, S.ctypes.data_as(dp), Q, ai.ctypes.data_as(dp), ptr(ti, dp), ptr(at, dp), P,
            int(seed) & (2 ** 64 - 1), self._mode(mode), ptr(r, ip) if NR else None, NR, ptr(qo, dp),
            ptr(band_th, dp) if NR else None, ptr(band_st, dp) if NR else None, tally.ctypes.data_as(ip), ptr(exceed, ip),
            ptr(th_all, dp), ptr(st_all, dp), ptr(words, ip), ptr(data, dp)))
        out = (band_th, band_st, tally) + ((exceed,) if qo is not None else ())
        return out + ((th_all, st_all, words, data) if raw else ())

    def inject_device(self, d_R_ptr, ntab, spectra, a_inj, P, seed, theta_inj=None, a_test=None, mode="two-sided",
                      ranks=None, q_obs=None, d_band_theta_ptr=None, d_band_stat_ptr=None, d_tally_ptr=None,
                      d_exceed_ptr=None, d_theta_all_ptr=None, d_stat_all_ptr=None, d_words_all_ptr=None,
                      d_data_all_ptr=None, stream_ptr=None, nuisance=None):
        """Asynchronous ``inject`` on device-resident folded matrices d_R [ntab][M][C]: the outputs are raw pointers
        (d_band_theta, d_band_stat [ntab][Q][NR], d_theta_all, d_stat_all [ntab][Q][P] and d_data_all [ntab][Q][P][C]
        doubles; d_tally [ntab][Q][4], d_exceed [ntab][Q] and d_words_all [ntab][Q][P][2] ints), any may be 0 / None; with
        ranks one band is needed, and d_exceed comes with q_obs.  ranks: ints (None: detector.band_ranks(P); an empty
        list: no band).  The other arguments are host data and are copied.  nuisance: as for ``inject``.  Returns (Q, NR)."""
        self._nuisance(nuisance)
        S, ai, ti, at, r, qo = self._inject_args(spectra, a_inj, theta_inj, a_test, ranks, P, q_obs, int(ntab))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        vp = ctypes.c_void_p

        def ptr(x, t):
            return x.ctypes.data_as(t) if x is not None else None

        def dev(x):
            return vp(x) if x else None
        _lib.check(_lib.load().nusi_plan_response_inject(
            self._h, vp(d_R_ptr), int(ntab), S.ctypes.data_as(dp), len(S), ai.ctypes.data_as(dp), ptr(ti, dp), ptr(at, dp),
            int(P), int(seed) & (2 ** 64 - 1), self._mode(mode), ptr(r, ip) if len(r) else None, len(r), ptr(qo, dp),
            dev(d_band_theta_ptr), dev(d_band_stat_ptr), dev(d_tally_ptr), dev(d_exceed_ptr), dev(d_theta_all_ptr),
            dev(d_stat_all_ptr), dev(d_words_all_ptr), dev(d_data_all_ptr), dev(stream_ptr)))
        return len(S), len(r)

    # --- the toy-calibrated interval (include/nusi.h nusi_plan_response_belt) ---
    def _belt_args(self, spectra, data, frac, ref, ntab):
        S, _ = self._spectra(spectra, None)
        d = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
        C = self.detector_bins()
        if C and d.shape != (C,):                                   # (no detector: the library refuses, NUSI_ESTATE)
            raise ValueError("belt: data must have shape (%d,), got %s" % (C, np.shape(data)))
        fr = np.ascontiguousarray(frac, dtype=np.float64).reshape(-1)
        rf = None
        if ref is not None:
            rf = np.asarray(ref, dtype=np.float64)
            if rf.ndim == 1:                                        # (Q,): one reference per spectrum, every table
                rf = rf[None, :]
            rf = np.ascontiguousarray(np.broadcast_to(rf, (ntab, len(S))))
        return S, d, fr, rf

    def belt(self, R, spectra, data, frac, P, seed, ref=None, mode="two-sided", alpha=0.1, raw=False, nuisance=None):
        """The toy-calibrated confidence interval of the signal's scale -- the Feldman-Cousins interval by the profile
        construction -- on a grid of test scales, in one call on the GPU.  Per table t, spectrum q and grid point g the
        test scale is a = frac[g] * ref[t, q]; the data (C,) get ``inject``'s steps at a (``fit`` / ``profile``,
        ``fit_fixed``, the statistic), which gives the observed records and q_obs; P toys are drawn on the device from
        the conditional fit's own expectation (stream = t, row = q G + g) and each gets the same steps at a; a point is
        accepted iff exceed > alpha * (P - tally[0] - tally[1]).  frac: (G,), finite, >= 0, strictly ascending, G <=
        _lib.BELT_GRID_MAX.  ref: None (1), a number, (Q,) or (ntab, Q) -- e.g. ``limit``'s upper limit; NaN, infinite
        or negative: BELT_NO_GRID.  mode: "two-sided" or "upper".  Returns detector.belt_host's tuple: (lo (ntab, Q), hi
        (ntab, Q), idx (ntab, Q, 2) int32, status (ntab, Q) int32 -- _lib.BELT_* --, exceed (ntab, Q, G) int32, tally
        (ntab, Q, G, 4) int32, q_obs (ntab, Q, G), theta_obs (ntab, Q, 1 + G, 1 + K), words_obs (ntab, Q, 1 + G) int32)
        and with raw also (theta_all (ntab, Q, G, P), stat_all (ntab, Q, G, P), words_all (ntab, Q, G, P, 2) int32,
        data_all (ntab, Q, G, P, C)).  No axis is squeezed.

        nuisance: "fixed" or "global" (the prior means redrawn per toy around the observed conditional fit's theta_j(a),
        theta_obs[t, q, 1 + g, 1 + j]: ``draw_normal`` with stream = t at [q G + g, p, j]), as for ``inject``; under
        "prior" the call is refused."""
        self._nuisance(nuisance)
        R, C = self._folded(R, "belt")
        ntab, P = R.shape[0], int(P)
        S, d, fr, rf = self._belt_args(spectra, data, frac, ref, ntab)
        Q, G, NC, Pa = len(S), len(fr), self.templates() + 1, max(P, 0)
        lo, hi = np.full((ntab, Q), np.nan), np.full((ntab, Q), np.nan)
        idx, status = np.full((ntab, Q, 2), -1, dtype=np.int32), np.zeros((ntab, Q), dtype=np.int32)
        exceed, tally = np.zeros((ntab, Q, G), dtype=np.int32), np.zeros((ntab, Q, G, 4), dtype=np.int32)
        q_obs, th_obs = np.full((ntab, Q, G), np.nan), np.full((ntab, Q, 1 + G, NC), np.nan)
        w_obs = np.zeros((ntab, Q, 1 + G), dtype=np.int32)
        th_all = st_all = words = toys = None
        if raw:
            th_all, st_all = np.full((ntab, Q, G, Pa), np.nan), np.full((ntab, Q, G, Pa), np.nan)
            words, toys = np.zeros((ntab, Q, G, Pa, 2), dtype=np.int32), np.zeros((ntab, Q, G, Pa, C))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)

        def ptr(x, t):
            return x.ctypes.data_as(t) if x is not None else None
        _lib.check(_lib.load().nusi_plan_response_belt_host(
            self._h, R.ctypes.data_as(dp), ntab, S.ctypes.data_as(dp), Q, d.ctypes.data_as(dp), fr.ctypes.data_as(dp), G,
            ptr(rf, dp), P, int(seed) & (2 ** 64 - 1), self._mode(mode), float(alpha), ptr(lo, dp), ptr(hi, dp), ptr(idx, ip),
            ptr(status, ip), ptr(exceed, ip), ptr(tally, ip), ptr(q_obs, dp), ptr(th_obs, dp), ptr(w_obs, ip),
            ptr(th_all, dp), ptr(st_all, dp), ptr(words, ip), ptr(toys, dp)))
        out = (lo, hi, idx, status, exceed, tally, q_obs, th_obs, w_obs)
        return out + ((th_all, st_all, words, toys) if raw else ())

    def belt_device(self, d_R_ptr, ntab, spectra, data, frac, P, seed, ref=None, mode="two-sided", alpha=0.1,
                    d_lo_ptr=None, d_hi_ptr=None, d_idx_ptr=None, d_status_ptr=None, d_exceed_ptr=None, d_tally_ptr=None,
                    d_q_obs_ptr=None, d_theta_obs_ptr=None, d_words_obs_ptr=None, d_theta_all_ptr=None,
                    d_stat_all_ptr=None, d_words_all_ptr=None, d_data_all_ptr=None, stream_ptr=None, nuisance=None):
        """Asynchronous ``belt`` on device-resident folded matrices d_R [ntab][M][C]: the outputs are raw pointers (d_lo,
        d_hi [ntab][Q], d_q_obs [ntab][Q][G], d_theta_obs [ntab][Q][1 + G][1 + K], d_theta_all, d_stat_all
        [ntab][Q][G][P] and d_data_all [ntab][Q][G][P][C] doubles; d_idx [ntab][Q][2], d_status [ntab][Q], d_exceed
        [ntab][Q][G], d_tally [ntab][Q][G][4], d_words_obs [ntab][Q][1 + G] and d_words_all [ntab][Q][G][P][2] ints), any
        may be 0 / None but not all.  The other arguments are host data and are copied.  nuisance: as for ``belt``.
        Returns (Q, G)."""
        self._nuisance(nuisance)
        S, d, fr, rf = self._belt_args(spectra, data, frac, ref, int(ntab))
        dp = ctypes.POINTER(ctypes.c_double)
        vp = ctypes.c_void_p

        def dev(x):
            return vp(x) if x else None
        _lib.check(_lib.load().nusi_plan_response_belt(
            self._h, vp(d_R_ptr), int(ntab), S.ctypes.data_as(dp), len(S), d.ctypes.data_as(dp), fr.ctypes.data_as(dp),
            len(fr), rf.ctypes.data_as(dp) if rf is not None else None, int(P), int(seed) & (2 ** 64 - 1), self._mode(mode),
            float(alpha), dev(d_lo_ptr), dev(d_hi_ptr), dev(d_idx_ptr), dev(d_status_ptr), dev(d_exceed_ptr),
            dev(d_tally_ptr), dev(d_q_obs_ptr), dev(d_theta_obs_ptr), dev(d_words_obs_ptr), dev(d_theta_all_ptr),
            dev(d_stat_all_ptr), dev(d_words_all_ptr), dev(d_data_all_ptr), dev(stream_ptr)))
        return len(S), len(fr)

    # --- the toy-calibrated region of the flavour composition (include/nusi.h nusi_plan_response_composition_belt) ---
    def _composition_args(self, spectra, data, phi, ntab):
        S, _ = self._spectra(spectra, None)
        d = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
        C = self.detector_bins()
        if C and d.shape != (C,):                                   # (no detector: the library refuses, NUSI_ESTATE)
            raise ValueError("composition_belt: data must have shape (%d,), got %s" % (C, np.shape(data)))
        ph = np.ascontiguousarray(phi, dtype=np.float64)
        if ph.ndim not in (2, 3) or ph.shape[-1] != 3 or (ph.ndim == 3 and ph.shape[0] != ntab):
            raise ValueError("composition_belt: phi must have shape (G, 3) or (ntab, G, 3), got %s" % (ph.shape,))
        return S, d, ph

    def composition_belt(self, R3, spectra, data, phi, P, seed, alpha=0.1, raw=False):
        """The toy-calibrated confidence region of the source's flavour composition -- the Feldman-Cousins region by
        the profile construction -- on a grid of compositions, in one call on the GPU.  R3 (ntab, 3, M, C): three folded
        rows per table, ``fit_components``' input; phi (G, 3) or (ntab, G, 3): weights >= 0 on those rows, no point all
        zeros, G <= _lib.REGION_GRID_MAX.  Per table t, spectrum q and point g the data (C,) get ``composition_scan``'s
        steps at phi_g -- the free fit of the three components, the fit on the composed rows with the scale and the
        plan's templates floating, the statistic --, which gives the observed records and q_obs; P toys are drawn on the
        device from the held fit's own expectation (``draw`` with stream = t at row q G + g) and each gets the same steps
        at phi_g; a point is accepted iff exceed > alpha * (P - tally[0] - tally[1]).  Returns
        detector.composition_belt_host's tuple: (accept (ntab, Q, G) bool, status (ntab, Q) int32 -- _lib.REGION_* --,
        best (ntab, Q) int32, exceed (ntab, Q, G) int32, tally (ntab, Q, G, 4) int32, q_obs (ntab, Q, G), theta_obs (ntab,
        Q, 1 + G, 3 + K), words_obs (ntab, Q, 1 + G) int32) and with raw also (theta_all (ntab, Q, G, P, 3 + K), stat_all
        (ntab, Q, G, P), words_all (ntab, Q, G, P, 2) int32, data_all (ntab, Q, G, P, C)).  No axis is squeezed.  Only
        the "fixed" toy ensemble is built: under another (``set_option(OPT_TOY_NUISANCE, ..)``) with a constrained
        template the call is refused."""
        R3, J, C = self._stack(R3, "composition_belt")
        if J != 3:
            raise ValueError("composition_belt: R3 must have shape (ntab, 3, M, C), got %s" % (R3.shape,))
        ntab, P = R3.shape[0], int(P)
        S, d, ph = self._composition_args(spectra, data, phi, ntab)
        Q, G, NC, Pa = len(S), ph.shape[-2], self.templates() + 3, max(P, 0)
        accept, status = np.zeros((ntab, Q, G), dtype=np.int32), np.zeros((ntab, Q), dtype=np.int32)
        best = np.full((ntab, Q), -1, dtype=np.int32)
        exceed, tally = np.zeros((ntab, Q, G), dtype=np.int32), np.zeros((ntab, Q, G, 4), dtype=np.int32)
        q_obs, th_obs = np.full((ntab, Q, G), np.nan), np.full((ntab, Q, 1 + G, NC), np.nan)
        w_obs = np.zeros((ntab, Q, 1 + G), dtype=np.int32)
        th_all = st_all = words = toys = None
        if raw:
            th_all, st_all = np.full((ntab, Q, G, Pa, NC), np.nan), np.full((ntab, Q, G, Pa), np.nan)
            words, toys = np.zeros((ntab, Q, G, Pa, 2), dtype=np.int32), np.zeros((ntab, Q, G, Pa, C))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)

        def ptr(x, t):
            return x.ctypes.data_as(t) if x is not None else None
        _lib.check(_lib.load().nusi_plan_response_composition_belt_host(
            self._h, R3.ctypes.data_as(dp), ntab, S.ctypes.data_as(dp), Q, d.ctypes.data_as(dp), ph.ctypes.data_as(dp),
            1 if ph.ndim == 3 else 0, G, P, int(seed) & (2 ** 64 - 1), float(alpha), ptr(accept, ip), ptr(status, ip),
            ptr(best, ip), ptr(exceed, ip), ptr(tally, ip), ptr(q_obs, dp), ptr(th_obs, dp), ptr(w_obs, ip),
            ptr(th_all, dp), ptr(st_all, dp), ptr(words, ip), ptr(toys, dp)))
        out = (accept != 0, status, best, exceed, tally, q_obs, th_obs, w_obs)
        return out + ((th_all, st_all, words, toys) if raw else ())

    def composition_belt_device(self, d_R3_ptr, ntab, spectra, data, phi, P, seed, alpha=0.1, d_accept_ptr=None,
                                d_status_ptr=None, d_best_ptr=None, d_exceed_ptr=None, d_tally_ptr=None, d_q_obs_ptr=None,
                                d_theta_obs_ptr=None, d_words_obs_ptr=None, d_theta_all_ptr=None, d_stat_all_ptr=None,
                                d_words_all_ptr=None, d_data_all_ptr=None, stream_ptr=None):
        """Asynchronous ``composition_belt`` on a device-resident stack d_R3 [ntab][3][M][C]: the outputs are raw pointers
        (d_q_obs [ntab][Q][G], d_theta_obs [ntab][Q][1 + G][3 + K], d_theta_all [ntab][Q][G][P][3 + K], d_stat_all
        [ntab][Q][G][P] and d_data_all [ntab][Q][G][P][C] doubles; d_accept [ntab][Q][G], d_status, d_best [ntab][Q],
        d_exceed [ntab][Q][G], d_tally [ntab][Q][G][4], d_words_obs [ntab][Q][1 + G] and d_words_all [ntab][Q][G][P][2]
        ints), any may be 0 / None but not all; d_accept, d_status and d_best need d_exceed, d_tally, d_q_obs and
        d_words_obs.  The other arguments are host data and are copied.  Returns (Q, G)."""
        S, d, ph = self._composition_args(spectra, data, phi, int(ntab))
        dp = ctypes.POINTER(ctypes.c_double)
        vp = ctypes.c_void_p

        def dev(x):
            return vp(x) if x else None
        _lib.check(_lib.load().nusi_plan_response_composition_belt(
            self._h, vp(d_R3_ptr), int(ntab), S.ctypes.data_as(dp), len(S), d.ctypes.data_as(dp), ph.ctypes.data_as(dp),
            1 if ph.ndim == 3 else 0, ph.shape[-2], int(P), int(seed) & (2 ** 64 - 1), float(alpha), dev(d_accept_ptr),
            dev(d_status_ptr), dev(d_best_ptr), dev(d_exceed_ptr), dev(d_tally_ptr), dev(d_q_obs_ptr), dev(d_theta_obs_ptr),
            dev(d_words_obs_ptr), dev(d_theta_all_ptr), dev(d_stat_all_ptr), dev(d_words_all_ptr), dev(d_data_all_ptr),
            dev(stream_ptr)))
        return len(S), ph.shape[-2]

    def set_cascade(self, kind):
        """Cascade kernel of later calls: _lib.CASCADE_AUTO (default) = CASCADE_MFMA (the wavefront with its push
        on the fp64 matrix cores, the block-synchronous k_cascade_bs), or CASCADE_{WAVEFRONT,REG,LDS} (since
        round 5 all three the bit-exact scalar kernel k_cascade)."""
        _lib.check(_lib.load().nusi_plan_set_cascade(self._h, int(kind)))

    def set_option(self, option, value):
        """A/B and test options (nusi_plan_set_option): _lib.OPT_ALPHA_BATCH (max tables per alpha batch, 0 =
        auto), OPT_ALPHA_KERNEL (0 batch, 1 tile, 2 per entry), OPT_CASCADE_RHS (1 = one point per cascade
        workgroup), OPT_STEP_PASSES (1 = the step-pass cascade also where one pass fits), OPT_SHIFT_REUSE (K > 0:
        the opt-in scan mode sharing tables across m_phi on the r^(-o/2) lattice, o <= K; only tables with g <= 0.05
        share, the others are built directly), OPT_REFERENCE_ORDER (1, the default = the tables in the reference's own
        arithmetic: GSL's dilogarithm algorithms on the reference's arguments; 0 = the shared-algorithm order), OPT_REFO_CORNER_MB (the reference order's
        member-corner block budget in MiB, 0 = automatic), OPT_GA_BATCH (the reference order's Gamma / alphaTilde path:
        0 auto, 1 the per-table kernel, 2 the batch path whenever batches exist), OPT_GA_PRE_MB (the batch path's block
        budget in MiB, 0 = 512; OPT_GA_PRE_KB: the same in KiB), OPT_RESPONSE_FIFO_KB (the response's impulse
        cascade: its step-pass FIFO budget in KiB, 0 = 1 GiB; the tables run in chunks that fit), OPT_ENSEMBLE_QSLICES
        and OPT_ENSEMBLE_PSLICES (``ensemble``'s grid is (tables, q-slices, p-slices): 0 = automatic, n >= 1 = exactly
        min(n, what there is to split); any value gives the same bits), OPT_ENSEMBLE_LIMIT_MB (``ensemble_limit``'s
        scratch budget in MiB, 0 = 256; the call runs in chunks that fit; OPT_ENSEMBLE_LIMIT_BYTES: the same in bytes),
        OPT_TOY_NUISANCE (the toys of ``inject`` and ``belt``: TOYS_FIXED, TOYS_GLOBAL or TOYS_PRIOR); include/nusi.h."""
        _lib.check(_lib.load().nusi_plan_set_option(self._h, int(option), int(value)))

    def profile_begin(self, max_calls):
        _lib.check(_lib.load().nusi_plan_profile_begin(self._h, int(max_calls)))

    def profile_end(self):
        """Summed kernel ms [gamma/alphaTilde, alpha, cascade] and the number of calls recorded."""
        ms = (ctypes.c_double * 3)()
        n = ctypes.c_int()
        _lib.check(_lib.load().nusi_plan_profile_end(self._h, ms, ctypes.byref(n)))
        return list(ms), n.value

    def stage_ms(self):
        ms = (ctypes.c_float * 3)()
        _lib.check(_lib.load().nusi_plan_stage_ms(self._h, ms))
        return list(ms)

    def warnings(self, n):
        out = (ctypes.c_int * n)()
        _lib.check(_lib.load().nusi_plan_warnings(self._h, out, n))
        return list(out)

    def kernels(self):
        """(alpha-table kernel, cascade kernel) the last call launched, e.g. ('k_alpha_batch', 'k_cascade_bs')."""
        a, c = ctypes.c_char_p(), ctypes.c_char_p()
        _lib.check(_lib.load().nusi_plan_kernels(self._h, ctypes.byref(a), ctypes.byref(c)))
        return a.value.decode(), c.value.decode()

    def ga_kernel(self):
        """The Gamma / alphaTilde path of the last call, e.g. 'k_ga_dilogs_batch + k_gamma_alphat[pre]'."""
        g = ctypes.c_char_p()
        _lib.check(_lib.load().nusi_plan_ga_kernel(self._h, ctypes.byref(g)))
        return g.value.decode()

    def tables(self, i):
        """Point i's Stage-A tables of the last call: Gamma[T], alphaTilde[T], alpha packed [T(T-1)/2]."""
        G, At, A = np.zeros(self.T), np.zeros(self.T), np.zeros(self.PT)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().nusi_plan_tables(self._h, int(i), G.ctypes.data_as(dp), At.ctypes.data_as(dp),
                                                A.ctypes.data_as(dp)))
        return G, At, A


def unpack_alpha(A_packed, T):
    """packed transposed alpha (m(m-1)/2+n) -> dense T x T with alpha[n, m], n < m."""
    out = np.zeros((T, T))
    m_idx, n_idx = np.tril_indices(T, -1)       # row-major over m, n < m -> m(m-1)/2 + n order
    out[n_idx, m_idx] = A_packed
    return out
