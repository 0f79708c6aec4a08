"""Response matrices on the CPU (numpy only): the yardstick of nusi_plan_response_apply.

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
