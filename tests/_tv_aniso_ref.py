"""The float64 reference of the anisotropic TV prior, g(x) = ||d_r x||_1 + ||d_c x||_1: its value and its prox, shared by tests/test_gpu_tv_aniso.py and
tests/_mala_ref.py.  numpy only."""
import numpy as np

from oracle import lmc_oracle as O


def tv_prox_aniso(x, gamma, niter, step=0.125, momentum="unlocbox"):
    """prox_{gamma TV_aniso}(x): `niter` FGP dual updates from the zero dual, then x - gamma div(rr, ss); images on the last two axes."""
    x = np.asarray(x)
    dt = x.dtype
    gamma = dt.type(gamma)
    c = dt.type(step) / gamma
    betas = np.asarray(O.fgp_betas(niter, momentum), dtype=dt)
    rr, ss, p, q = (np.zeros_like(x) for _ in range(4))
    one = dt.type(1)
    for k in range(niter):
        dr, dc = O.grad2d(x - gamma * O.div2d(rr, ss))
        pn, qn = np.clip(rr - c * dr, -one, one), np.clip(ss - c * dc, -one, one)
        rr, ss = pn + betas[k] * (pn - p), qn + betas[k] * (qn - q)
        p, q = pn, qn
    return x - gamma * O.div2d(rr, ss)


def tv_aniso_value(x):
    dr, dc = O.grad2d(x)
    return np.sum(np.abs(dr) + np.abs(dc), axis=(-2, -1))
