"""The SE(3) angle tests' own yardstick: exp as torch.linalg.matrix_exp of the 4x4 twist in fp64, a unit quaternion as a rotation
matrix by explicit algebra, and the sweep of rotation angles the tests run on.  None of pvo_amd.geom.se3's formulas are used: no
series, no closed forms in theta, no cutoffs.  Everything here is differentiable by autograd, which is what the gradient tests hold
the kernels' and the torch formulation's vector-Jacobian products to."""
import math

import torch

# every branch of exp / log and the band between lietorch's switch (1e-6) and the angles the other tests use (>= 1e-2)
ANGLES = (0.0, 1e-8, 1e-7, 5e-7, 9.9e-7, 1.01e-6, 1.5e-6, 1e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.5, 1.0, 3.0, math.pi - 1e-3)


def twist(xi):
    """[..., 6] (tau, phi), lietorch's ordering -> the 4x4 twist [[hat(phi), tau], [0, 0]]"""
    tx, ty, tz, px, py, pz = xi.unbind(-1)
    z = torch.zeros_like(tx)
    return torch.stack([torch.stack([z, -pz, py, tx], -1), torch.stack([pz, z, -px, ty], -1),
                        torch.stack([-py, px, z, tz], -1), torch.stack([z, z, z, z], -1)], -2)


def exp_ref(xi):
    """-> (the 4x4 matrix of Exp(xi), its translation column), fp64.  The twist is balanced first: exp(T) = D exp(D^-1 T D) D^-1 with
    D = diag(1, 1, 1, s), s the power of two at or above max(1, |tau|), which is exact.  matrix_exp scales and squares, and its error
    grows with the norm of its argument: against mpmath at 40 digits, 2e-15 |tau| at |tau| = 30 unbalanced (more than the tests'
    fp64 bound of 1.8e-15 |tau|) and 4e-16 |tau| balanced, which test_se3_angles.test_reference_against_multiprecision asserts."""
    xi = xi.double()
    s = torch.exp2(torch.ceil(torch.log2(xi[..., :3].detach().norm(dim=-1, keepdim=True).clamp(min=1.0))))
    M = torch.linalg.matrix_exp(twist(torch.cat([xi[..., :3] / s, xi[..., 3:]], -1)))
    M = torch.cat([M[..., :3], M[..., 3:] * torch.cat([s, s, s, torch.ones_like(s)], -1)[..., None]], -1)
    return M, M[..., :3, 3]


def quat_matrix(q):
    """quaternion (x, y, z, w) -> rotation matrix, fp64: the homogeneous form, exact for any nonzero q"""
    x, y, z, w = q.double().unbind(-1)
    s = 2.0 / (x * x + y * y + z * z + w * w)
    return torch.stack([torch.stack([1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)], -1),
                        torch.stack([s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)], -1),
                        torch.stack([s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)], -1)], -2)


def pose_matrix(g):
    """[..., 7] (t, q) -> the 4x4 matrix, fp64"""
    R, t = quat_matrix(g[..., 3:]), g[..., :3].double()
    top = torch.cat([R, t[..., None]], -1)
    bottom = torch.zeros_like(top[..., :1, :])
    bottom[..., 3] = 1.0
    return torch.cat([top, bottom], -2)


def angles(extra=()):
    """ANGLES followed by both sides (1 -+ 1 %) of each cutoff in `extra`"""
    out = list(ANGLES)
    for c in extra:
        out += [0.99 * c, 1.01 * c]
    return out


def sweep(n=64, seed=0, extra=()):
    """-> xi [A, n, 6] fp64: per angle of angles(extra), n unit directions times the angle; tau ~ N(0, I) for the first half of the
    rows and 10 N(0, I) for the second.  Directions and translations are the same at every angle."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=-1, keepdim=True)
    tau = torch.randn(n, 3, generator=g, dtype=torch.float64)
    tau[n // 2:] *= 10.0
    th = torch.tensor(angles(extra), dtype=torch.float64)
    return torch.cat([tau.expand(th.shape[0], n, 3), th[:, None, None] * d], -1).contiguous()
