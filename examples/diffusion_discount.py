#!/usr/bin/env python3
"""Discounted anisotropic diffusion, phi_t = trace(sigma D^2phi sigma^T) - lambda phi, as a ToolboxLS script writes it: termSum
of termTraceHessian (L = sigma, R = sigma^T) and termDiscount, integrated with odeCFL3 on device tensors.

    python examples/diffusion_discount.py [n] [t_end]

This is the Feynman-Kac form of E[exp(-lambda t) phi0(X_t)] for dX = sqrt(2) sigma^T dW.  A normalised Gaussian spreads
along sigma^T sigma and decays: its mass is exp(-lambda t) and its covariance Sigma0 + 2 sigma^T sigma t.  Needs an MI355X.
Prints both against those closed forms at a few instants; the state never leaves the GPU.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                    # noqa: E402
import levelsetpy_amd as lsp    # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 161
t_end = float(sys.argv[2]) if len(sys.argv) > 2 else 0.2

sigma = np.array([[0.6, 0.2], [-0.1, 0.4]])
lam = 1.5
S0 = np.array([[0.2, 0.05], [0.05, 0.12]])

g = lsp.createGrid(-3 * np.ones((2, 1)), 3 * np.ones((2, 1)), n * np.ones((2, 1), dtype=np.int64))
X = np.stack(g.xs).reshape(2, -1)
cell = float(np.prod(np.asarray(g.dx).ravel()))
data0 = np.exp(-0.5 * np.einsum('ik,ij,jk->k', X, np.linalg.inv(S0), X))
data0 /= data0.sum() * cell

diffusion = lsp.Bundle(dict(grid=g, hessianFunc=lsp.hessianSecond, L=sigma, R=sigma.T))
discount = lsp.Bundle(dict(grid=g, lambder=lam))
schemeData = lsp.Bundle(dict(grid=g, innerFunc=[lsp.termTraceHessian, lsp.termDiscount], innerData=[diffusion, discount]))
options = lsp.odeCFLset(lsp.Bundle(dict(factorCFL=0.5)))

phi = torch.as_tensor(data0.reshape(-1, 1), device="cuda")
Xd = torch.as_tensor(X, device="cuda")
t = 0.0
t0 = time.perf_counter()
for t_next in np.linspace(0, t_end, 5)[1:]:
    t, phi, schemeData = lsp.odeCFL3(lsp.termSum, [t, float(t_next)], phi, options, schemeData)
    w = phi.reshape(-1)
    mass = float(w.sum()) * cell
    mu = (Xd * w).sum(1) / w.sum()
    cov = ((Xd * w) @ Xd.T / w.sum() - torch.outer(mu, mu)).cpu().numpy()
    want = S0 + 2 * sigma.T @ sigma * t
    print("t = %.3f  mass %.6f (exp(-lambda t) %.6f)  max |cov - (Sigma0 + 2 sigma^T sigma t)| %.1e  (%s, %.2f s)"
          % (t, mass, np.exp(-lam * t), float(np.abs(cov - want).max()), phi.device, time.perf_counter() - t0))
