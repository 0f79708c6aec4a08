"""ctypes binding of libnusi.so (include/nusi.h).

The library is built in-tree (``make -C nusiprop_amd/csrc``) and loaded from
this directory; there is no pure-Python or CPU fallback: if the .so is missing
or the GPU is unusable, calls raise.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NUSIPROP_LIB") or os.path.join(HERE, "libnusi.so")   # override: A/B builds only

NUSI_OK = 0
NUSI_EPARAM = -1
NUSI_ENOSPECTRUM = -2
NUSI_ETABLE = -3
NUSI_EINTERP = -4
NUSI_EHIP = -5
NUSI_ESTATE = -6

SOURCE_DSNB = 0
SOURCE_POWER_LAW = 1
SOURCE_TABULATED = 2        # + slot: a user-tabulated source of the plan (Plan.set_source, nusiprop_amd.sources)
SOURCE_SLOTS_MAX = 65536
DETECTOR_BINS_MAX = 64      # reconstructed bins of a plan's detector (Plan.set_detector, nusiprop_amd.detector)
# the status word of Plan.profile (NUSI_FIT_*): the step count in the low 8 bits, flags above
FIT_ITER_MAX = 64
FIT_STEPS_MASK = 0xFF
FIT_FLAT, FIT_BOUNDARY, FIT_NOT_CONVERGED, FIT_INFINITE = 0x100, 0x200, 0x400, 0x800
# ... and of Plan.fit: a singular Newton system, FIT_ZERO << j for a component that ends at zero, the halvings from bit 24
FIT_TEMPLATES_MAX = 3
FIT_SIGNALS_MAX = 3         # the signal components of Plan.fit_components
FIT_TRIALS_MAX = 64
FIT_SINGULAR, FIT_ZERO, FIT_TRIALS_SHIFT, FIT_TRIALS_MASK = 0x1000, 0x10000, 24, 0x7F
# Plan.limit (NUSI_LIMIT_*): the sides, the outer cap, and a side's status word: the outer steps in the low 8 bits, the flags,
# the inner Newton steps (saturating) from bit 16
LIMIT_LOWER, LIMIT_UPPER = 1, 2
LIMIT_ITER_MAX = 64
LIMIT_STEPS_MASK = 0xFF
LIMIT_AT_ZERO, LIMIT_UNBOUNDED, LIMIT_NO_FIT, LIMIT_NOT_CONVERGED = 0x100, 0x200, 0x400, 0x800
LIMIT_INNER_SHIFT, LIMIT_INNER_MASK = 16, 0x7FFF

WARN_GAMMA = 1
WARN_ALPHATILDE = 2
WARN_ALPHA = 4


class NusiParams(ctypes.Structure):
    """struct nusi_params -- the calculate_flux constructor arguments (nuSIprop.hpp:61-65)."""
    _fields_ = [("mphi", ctypes.c_double), ("g", ctypes.c_double), ("mntot", ctypes.c_double),
                ("si", ctypes.c_double), ("norm", ctypes.c_double),
                ("majorana", ctypes.c_int), ("non_resonant", ctypes.c_int), ("normal_ordering", ctypes.c_int),
                ("N_bins_E", ctypes.c_int), ("lEmin", ctypes.c_double), ("lEmax", ctypes.c_double),
                ("zmax", ctypes.c_double), ("flav", ctypes.c_int), ("phiphi", ctypes.c_int),
                ("source_model", ctypes.c_int)]


class NusiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


# every symbol declared in include/nusi.h (tests/test_capi_symbols.py checks this list against the header)
EXPORTS = [
    "nusi_params_default", "nusi_last_error", "nusi_device_count",
    "nusi_create", "nusi_copy", "nusi_destroy", "nusi_set_params", "nusi_get_params", "nusi_evolve",
    "nusi_check_energy_conservation", "nusi_get_flux", "nusi_get_flux_fla", "nusi_get_energies",
    "nusi_get_N_bins_E", "nusi_get_N_steps_z", "nusi_get_warnings", "nusi_get_kernels", "nusi_set_option",
    "nusi_plan_create", "nusi_plan_destroy", "nusi_plan_load_phiphi", "nusi_plan_grid", "nusi_plan_evolve",
    "nusi_plan_evolve_host", "nusi_plan_stage_ms", "nusi_plan_profile_begin", "nusi_plan_profile_end",
    "nusi_plan_warnings", "nusi_plan_tables", "nusi_evolve_batch", "nusi_plan_set_cascade",
    "nusi_plan_kernels", "nusi_plan_ga_kernel", "nusi_plan_set_option",
    "nusi_plan_source_axis", "nusi_plan_set_source", "nusi_source_axis", "nusi_set_source",
    "nusi_plan_response", "nusi_plan_response_host", "nusi_plan_response_apply", "nusi_plan_response_apply_host",
    "nusi_response",
    "nusi_mixing", "nusi_mass_fractions", "nusi_response_mass_shape", "nusi_plan_step_constants",
    "nusi_plan_response_mass", "nusi_plan_response_mass_host", "nusi_plan_response_compose",
    "nusi_plan_response_compose_host", "nusi_response_mass",
    "nusi_plan_set_detector", "nusi_plan_detector_bins", "nusi_plan_fold_flux", "nusi_plan_fold_flux_host",
    "nusi_plan_response_fold", "nusi_plan_response_fold_host", "nusi_plan_response_events",
    "nusi_plan_response_events_host", "nusi_plan_response_profile", "nusi_plan_response_profile_host",
    "nusi_plan_set_templates", "nusi_plan_templates", "nusi_plan_response_fit", "nusi_plan_response_fit_host",
    "nusi_fit_components_shape", "nusi_plan_response_fit_components", "nusi_plan_response_fit_components_host",
    "nusi_plan_response_fit_fixed", "nusi_plan_response_fit_fixed_host",
    "nusi_plan_response_limit", "nusi_plan_response_limit_host",
    "nusi_plan_response_ensemble", "nusi_plan_response_ensemble_host",
    "nusi_plan_response_ensemble_limit", "nusi_plan_response_ensemble_limit_host",
    "nusi_plan_draw_counts", "nusi_plan_draw_counts_host",
    "nusi_plan_draw_normals", "nusi_plan_draw_normals_host",
    "nusi_plan_response_inject", "nusi_plan_response_inject_host",
    "nusi_belt_shape", "nusi_plan_response_belt", "nusi_plan_response_belt_host",
    "nusi_composition_belt_shape", "nusi_plan_response_composition_belt", "nusi_plan_response_composition_belt_host",
]

# nusi_plan_set_cascade kinds and nusi_plan_set_option options (include/nusi.h)
CASCADE_AUTO, CASCADE_WAVEFRONT, CASCADE_REG, CASCADE_LDS, CASCADE_MFMA = 0, 1, 2, 3, 4
OPT_ALPHA_BATCH, OPT_ALPHA_KERNEL, OPT_CASCADE_RHS, OPT_STEP_PASSES, OPT_SHIFT_REUSE = 1, 2, 3, 4, 5
OPT_REFERENCE_ORDER = 6
OPT_CASCADE_SYNC = 7
OPT_REFO_CORNER_MB = 8
OPT_GA_BATCH, OPT_GA_PRE_MB, OPT_GA_PRE_KB = 9, 10, 11
OPT_RESPONSE_FIFO_KB = 12
OPT_ENSEMBLE_QSLICES, OPT_ENSEMBLE_PSLICES = 13, 14    # Plan.ensemble's grid (tables, q-slices, p-slices); 0 = automatic
ENSEMBLE_DATASETS_MAX = 65536
# Plan.ensemble_limit: its scratch budget in MiB (0 = 256) or, where > 0, in bytes; the most ranks of a band and data sets
OPT_ENSEMBLE_LIMIT_MB, OPT_ENSEMBLE_LIMIT_BYTES = 15, 16
# the toys of Plan.inject and Plan.belt under a prior (include/nusi.h NUSI_OPT_TOY_NUISANCE, NUSI_TOYS_*): the prior means
# stay, are redrawn per toy (global observables), or the nuisances are thrown from the priors (inject only)
OPT_TOY_NUISANCE = 17
TOYS_FIXED, TOYS_GLOBAL, TOYS_PRIOR = 0, 1, 2
NORMAL_ROUNDS = 64              # Plan.draw_normal: the rounds of the polar method before the draw is the center
BAND_RANKS_MAX = 16
BAND_DATASETS_MAX = 4096
INJECT_TWO_SIDED, INJECT_UPPER, INJECT_DISCOVERY = 0, 1, 2     # Plan.inject's mode (include/nusi.h NUSI_INJECT_*)
# Plan.belt: the most grid points and the status word's bits (include/nusi.h NUSI_BELT_*, detector.BELT_*)
BELT_GRID_MAX = 64
BELT_NO_GRID, BELT_NO_FIT, BELT_BAD_POINT, BELT_EMPTY, BELT_LO_EDGE, BELT_HI_EDGE, BELT_GAPS = 1, 2, 4, 8, 16, 32, 64
# Plan.composition_belt: the most points of the composition grid and the status word's bits (NUSI_REGION_*, detector.REGION_*)
REGION_GRID_MAX = 1024
REGION_NO_FIT, REGION_BAD_POINT, REGION_EMPTY, REGION_ALL = 1, 2, 4, 8
DRAW_DATASETS_MAX = 1 << 26     # Plan.draw: the toys per bin (the generator's counter holds p * 64 + c)
DRAW_COUNTS_MAX = ((1 << 31) - 1) * 256     # ... and the counts of a call, rows * P * C (one launch, 256 counts a block)

_lib = None


def load():
    """Load libnusi.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("nusiprop_amd: %s not built (run `make -C nusiprop_amd/csrc`)" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    d, i, vp = ctypes.c_double, ctypes.c_int, ctypes.c_void_p
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    pp = ctypes.POINTER(NusiParams)
    sig = {
        "nusi_params_default": (None, [pp, d, d, d, d]),
        "nusi_last_error": (ctypes.c_char_p, []),
        "nusi_device_count": (i, []),
        "nusi_create": (i, [pp, ctypes.POINTER(vp)]),
        "nusi_copy": (i, [vp, ctypes.POINTER(vp)]),
        "nusi_destroy": (None, [vp]),
        "nusi_set_params": (i, [vp, d, d, d, d, d]),
        "nusi_get_params": (i, [vp, dp]),
        "nusi_evolve": (i, [vp]),
        "nusi_check_energy_conservation": (i, [vp, dp]),
        "nusi_get_flux": (i, [vp, dp]),
        "nusi_get_flux_fla": (i, [vp, dp]),
        "nusi_get_energies": (i, [vp, dp]),
        "nusi_get_N_bins_E": (i, [vp]),
        "nusi_get_N_steps_z": (i, [vp]),
        "nusi_get_warnings": (i, [vp]),
        "nusi_get_kernels": (i, [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p)]),
        "nusi_set_option": (i, [vp, i, i]),
        "nusi_plan_create": (i, [i, i, d, d, d, i, ctypes.POINTER(vp)]),
        "nusi_plan_destroy": (None, [vp]),
        "nusi_plan_load_phiphi": (i, [vp, ctypes.c_char_p, ip, ctypes.c_char_p, ip]),
        "nusi_plan_grid": (i, [vp, ip, ip, dp]),
        "nusi_plan_evolve": (i, [vp, pp, i, vp, vp, vp]),
        "nusi_plan_evolve_host": (i, [vp, pp, i, dp, dp]),
        "nusi_plan_stage_ms": (i, [vp, ctypes.POINTER(ctypes.c_float)]),
        "nusi_plan_profile_begin": (i, [vp, i]),
        "nusi_plan_profile_end": (i, [vp, dp, ip]),
        "nusi_plan_warnings": (i, [vp, ip, i]),
        "nusi_plan_tables": (i, [vp, i, dp, dp, dp]),
        "nusi_evolve_batch": (i, [i, pp, i, dp, dp]),
        "nusi_plan_set_cascade": (i, [vp, i]),
        "nusi_plan_set_option": (i, [vp, i, i]),
        "nusi_plan_kernels": (i, [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p)]),
        "nusi_plan_ga_kernel": (i, [vp, ctypes.POINTER(ctypes.c_char_p)]),
        "nusi_plan_source_axis": (i, [vp, ip, dp, dp, dp]),
        "nusi_plan_set_source": (i, [vp, i, dp, dp]),
        "nusi_source_axis": (i, [vp, ip, dp, dp, dp]),
        "nusi_set_source": (i, [vp, dp, dp]),
        "nusi_plan_response": (i, [vp, pp, i, dp, vp, vp, vp]),
        "nusi_plan_response_host": (i, [vp, pp, i, dp, dp, dp]),
        "nusi_plan_response_apply": (i, [vp, vp, i, dp, i, dp, vp, vp]),
        "nusi_plan_response_apply_host": (i, [vp, dp, i, dp, i, dp, dp]),
        "nusi_response": (i, [vp, dp, dp, dp]),
        "nusi_mixing": (i, [i, dp]),
        "nusi_mass_fractions": (i, [i, dp, dp]),
        "nusi_response_mass_shape": (i, [i, i, i, ctypes.POINTER(ctypes.c_longlong)]),
        "nusi_plan_step_constants": (i, [vp, dp, dp]),
        "nusi_plan_response_mass": (i, [vp, pp, i, dp, vp, vp, vp]),
        "nusi_plan_response_mass_host": (i, [vp, pp, i, dp, dp, dp]),
        "nusi_plan_response_compose": (i, [vp, vp, i, ctypes.c_longlong, dp, i, vp, vp]),
        "nusi_plan_response_compose_host": (i, [vp, dp, i, ctypes.c_longlong, dp, i, dp]),
        "nusi_response_mass": (i, [vp, dp, dp, dp]),
        "nusi_plan_set_detector": (i, [vp, i, dp, dp]),
        "nusi_plan_detector_bins": (i, [vp]),
        "nusi_plan_fold_flux": (i, [vp, vp, i, vp, vp]),
        "nusi_plan_fold_flux_host": (i, [vp, dp, i, dp]),
        "nusi_plan_response_fold": (i, [vp, vp, i, vp, vp]),
        "nusi_plan_response_fold_host": (i, [vp, dp, i, dp]),
        "nusi_plan_response_events": (i, [vp, vp, i, dp, i, dp, dp, vp, vp, vp]),
        "nusi_plan_response_events_host": (i, [vp, dp, i, dp, i, dp, dp, dp, dp]),
        "nusi_plan_response_profile": (i, [vp, vp, i, dp, i, dp, vp, vp, vp, vp, vp]),
        "nusi_plan_response_profile_host": (i, [vp, dp, i, dp, i, dp, dp, dp, dp, ip]),
        "nusi_plan_set_templates": (i, [vp, i, dp, dp, dp]),
        "nusi_plan_templates": (i, [vp]),
        "nusi_plan_response_fit": (i, [vp, vp, i, dp, i, dp, vp, vp, vp, vp, vp]),
        "nusi_plan_response_fit_host": (i, [vp, dp, i, dp, i, dp, dp, dp, dp, ip]),
        "nusi_fit_components_shape": (i, [i, i, i, i, i, ctypes.POINTER(ctypes.c_longlong)]),
        "nusi_plan_response_fit_components": (i, [vp, vp, i, i, dp, i, dp, vp, vp, vp, vp, vp]),
        "nusi_plan_response_fit_components_host": (i, [vp, dp, i, i, dp, i, dp, dp, dp, dp, ip]),
        "nusi_plan_response_fit_fixed": (i, [vp, vp, i, dp, i, dp, dp, vp, vp, vp, vp, vp]),
        "nusi_plan_response_fit_fixed_host": (i, [vp, dp, i, dp, i, dp, dp, dp, dp, dp, ip]),
        "nusi_plan_response_limit": (i, [vp, vp, i, dp, i, dp, d, i, vp, vp, vp, vp, vp, vp]),
        "nusi_plan_response_limit_host": (i, [vp, dp, i, dp, i, dp, d, i, dp, dp, dp, dp, ip]),
        "nusi_plan_response_ensemble": (i, [vp, vp, i, dp, i, dp, i, vp, vp, vp, vp, vp]),
        "nusi_plan_response_ensemble_host": (i, [vp, dp, i, dp, i, dp, i, ip, dp, dp, ip]),
        "nusi_plan_response_ensemble_limit": (i, [vp, vp, i, dp, i, dp, i, d, i, ip, i, vp, vp, vp, vp, vp, vp, vp]),
        "nusi_plan_response_ensemble_limit_host": (i, [vp, dp, i, dp, i, dp, i, d, i, ip, i, dp, dp, ip, dp, dp, ip]),
        "nusi_plan_draw_counts": (i, [vp, dp, i, i, i, ctypes.c_ulonglong, ctypes.c_uint, vp, vp]),
        "nusi_plan_draw_counts_host": (i, [vp, dp, i, i, i, ctypes.c_ulonglong, ctypes.c_uint, dp]),
        "nusi_plan_draw_normals": (i, [vp, dp, dp, i, i, i, ctypes.c_ulonglong, ctypes.c_uint, vp, vp]),
        "nusi_plan_draw_normals_host": (i, [vp, dp, dp, i, i, i, ctypes.c_ulonglong, ctypes.c_uint, dp]),
        "nusi_plan_response_inject": (i, [vp, vp, i, dp, i, dp, dp, dp, i, ctypes.c_ulonglong, i, ip, i, dp,
                                          vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "nusi_plan_response_inject_host": (i, [vp, dp, i, dp, i, dp, dp, dp, i, ctypes.c_ulonglong, i, ip, i, dp,
                                               dp, dp, ip, ip, dp, dp, ip, dp]),
        "nusi_belt_shape": (i, [i, i, i, i, i, ctypes.POINTER(ctypes.c_longlong)]),
        "nusi_plan_response_belt": (i, [vp, vp, i, dp, i, dp, dp, i, dp, i, ctypes.c_ulonglong, i, d,
                                        vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "nusi_plan_response_belt_host": (i, [vp, dp, i, dp, i, dp, dp, i, dp, i, ctypes.c_ulonglong, i, d,
                                             dp, dp, ip, ip, ip, ip, dp, dp, ip, dp, dp, ip, dp]),
        "nusi_composition_belt_shape": (i, [i, i, i, i, i, i, ctypes.POINTER(ctypes.c_longlong)]),
        "nusi_plan_response_composition_belt": (i, [vp, vp, i, dp, i, dp, dp, i, i, i, ctypes.c_ulonglong, d,
                                                    vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "nusi_plan_response_composition_belt_host": (i, [vp, dp, i, dp, i, dp, dp, i, i, i, ctypes.c_ulonglong, d,
                                                         ip, ip, ip, ip, ip, dp, dp, ip, dp, dp, ip, dp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def last_error():
    return load().nusi_last_error().decode(errors="replace")


def check(code):
    if code != NUSI_OK:
        raise NusiError(code, load().nusi_last_error().decode(errors="replace"))
    return code


def make_params(mphi, g, mntot, si, norm=1.0, majorana=True, non_resonant=True, normal_ordering=True,
                N_bins_E=300, lEmin=12.0, lEmax=17.0, zmax=5.0, flav=2, phiphi=False,
                source_model=SOURCE_DSNB):
    return NusiParams(float(mphi), float(g), float(mntot), float(si), float(norm), int(bool(majorana)),
                      int(bool(non_resonant)), int(bool(normal_ordering)), int(N_bins_E), float(lEmin),
                      float(lEmax), float(zmax), int(flav), int(bool(phiphi)), int(source_model))
