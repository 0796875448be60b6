"""What tests/test_bnmemory_cpu.py and tests/test_gpu_bnmemory.py share: the contract of csrc/stil_bnmemory.h restated with ATen in
the input's dtype (memory_bn), DUA's momentum schedule in closed form, and the layer inputs of the entry-point tests, built on the
CPU so that the CPU test can show the GPU test's bar reachable on the very same numbers."""
import math
import os
import sys

import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_bnprior_cpu import blended_bn  # noqa: E402

MS = (1, 2, 49, 1000, 12544)
CS = (4, 64, 260, 2048)
# + one shape past 256 row tiles of 64 rows: the statistics take the two-launch (stage 1 + final) path there
SHAPES = [(M, C) for M in MS for C in CS] + [(64 * 257 + 3, 64)]
RHO_ALPHA = ((0.05, 0.05), (0.2, 0.5), (1.0, 0.1), (0.0, 1.0), (0.5, 0.0))
TOL = 2e-5   # close() of tests/test_gpu_bnprior.py: |a - b| <= TOL (1 + |b| + max|b|)


def memory_bn(x, gamma, beta, m, s, rho, alpha, unbiased, resid=None, relu=False, mask=None):
    """The forward of csrc/stil_bnmemory.h on rows x [M, C] in x's dtype: blended_bn with the memory (m, s) as the source, and the
    update.  -> (z, xhat, mu, r, delta, m', s')"""
    z, xhat, mu, r, delta = blended_bn(x, gamma, beta, m, s, rho, resid, relu, mask)
    M = x.shape[0]
    mu_b = x.mean(0)
    v_b = ((x - mu_b) ** 2).mean(0)
    c = M / (M - 1) if (unbiased and M > 1) else 1.0
    return z, xhat, mu, r, delta, (1 - alpha) * m + alpha * mu_b, (1 - alpha) * s + alpha * c * v_b


def momentum(alpha0, decay, amin, t):
    """alpha_t of the t-th update, t = 1, 2, ..."""
    return min(1.0, alpha0 * decay ** t + amin)


def layer_inputs(M, C):
    """One layer's tensors (CPU, float32), those of tests/test_gpu_bnprior.py's _Case: y = A W^T has |mean| / std = 50 per channel (a
    constant input column); the memory's mean sits 0.1 to 0.3 batch standard deviations off the batch mean, its variance within a
    factor 1.5 of the batch's, and mem_var[0] = 0 exactly (rstd reaches 1 / sqrt(eps) = 316 there at rho = 0).
    M = 2 is conditioned: the two rows differ in one input column alone, by 0.15 to 0.45 per channel (the standard deviation of the
    other shapes is 0.28), so no channel's batch variance is degenerate.  Two free rows leave some of 2048 channels with |y_1 - y_0| ~ 1e-3 std; there, at
    rho = 1, rstd -> 316 multiplies the float32 rounding of the statistics block's mean (half an ulp of 14 = 4.8e-7) into 1.5e-4 of z,
    past any float32 bar (float32 ATen misses 2e-5 by a factor 1.8 on such rows).  M = 1 has no such term: y - mean is exactly 0."""
    g = torch.Generator().manual_seed(1000 * M + C)
    K = 32
    A = torch.randn(M, K, generator=g)
    W = torch.randn(C, K, generator=g) * 0.05
    std = 0.05 * math.sqrt(K - 1)
    A[:, 0] = 1000.0
    W[:, 0] = 0.05 * std * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)   # mean = +-50 std
    if M == 2:
        A[1] = A[0]
        A[:, 1] = torch.tensor([3.0, -3.0])
        W[:, 1] = 0.05 * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0) * (0.5 + torch.rand(C, generator=g))   # |y_1 - y_0| in 0.15 .. 0.45
    y = A @ W.t()
    off = std * (0.1 + 0.2 * torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    rm = (y.double().mean(0) + off.double()).float()
    rv = std * std * (0.5 + torch.rand(C, generator=g))
    rv[0] = 0.0
    return dict(A=A, W=W, K=K, y=y, rm=rm, rv=rv, gamma=0.5 + torch.rand(C, generator=g), beta=0.2 * torch.randn(C, generator=g),
                resid=torch.randn(M, C, generator=g),
                rstats=torch.stack([torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g), 0.5 + torch.rand(C, generator=g),
                                    0.1 * torch.randn(C, generator=g)]).contiguous())
