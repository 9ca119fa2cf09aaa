"""What sets the series / closed-form cutoff of SE(3) exp and log (pvo_amd/csrc/se3_dual.h, pvo_amd/geom/se3.py): for trial cutoffs c,
the gradient errors of the torch formulation just above the cutoff (theta = 1.01 c, where the closed forms are worst), in units of the
type's unit roundoff u.  `log VJP`: the VJP of log(exp(xi)) against the cotangent it must return.  `exp VJP`: the VJP of exp's
translation against autograd through the fp64 matrix exponential (tests/se3_reference.py; its own noise is ~ 100 u of fp64).  Both are
relative to the largest entry, over 64 rows with |tau| up to 30, as tests/test_se3_angles.py measures them; its bound is 64 u.

    python tools/se3_cutoff.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import se3_reference as R
from pvo_amd.geom import se3 as S
from pvo_amd.geom.se3 import SE3


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def main():
    saved = dict(S.CUTOFF)
    try:
        for c in (0.02, 0.05, 0.1, 0.25, 0.5):
            for dt in (torch.float32, torch.float64):
                S.CUTOFF[dt] = c
                u = 0.5 * torch.finfo(dt).eps
                xi = R.sweep(64, 0, (c,))[-1:].to(dt)                          # theta = 1.01 c
                x, cot = xi.clone().requires_grad_(True), randn((1, 64, 6), 4).to(dt)
                g, = torch.autograd.grad((SE3.exp(x).log() * cot).sum(), x)
                log_vjp = ((g - cot).abs().max() / cot.abs().max()).item() / u
                xr, ct = xi.double().clone().requires_grad_(True), randn((1, 64, 3), 1)
                gr, = torch.autograd.grad((R.exp_ref(xr)[1] * ct).sum(), xr)
                x = xi.clone().requires_grad_(True)
                ge, = torch.autograd.grad((SE3.exp(x).data[..., :3].double() * ct).sum(), x)
                exp_vjp = ((ge.double() - gr).abs().max() / gr.abs().max()).item() / u
                print("cutoff %.2f %s: log VJP %5.0f u = %4.1f u / c    exp VJP %5.1f u = %4.1f u / c" %
                      (c, str(dt)[-7:], log_vjp, log_vjp * c, exp_vjp, exp_vjp * c))
    finally:
        S.CUTOFF.update(saved)


if __name__ == "__main__":
    main()
