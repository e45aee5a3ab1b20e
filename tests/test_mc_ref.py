"""CPU-only: the NumPy restatement of computeStochTrajs (tests/mc_ref.py) is what include/hj_mc.h states.

  * Philox4x32-10 in integer arithmetic gives the three published known answers;
  * with G = 0 a realisation is rollout_ref's trajectory, exactly, whatever the normals;
  * the discrete linear SDE: on the double integrator with u_bound = 0 the scheme is x1 += h x2 + g1 sqrt(h) xi, x2 += g2 sqrt(h) xi',
    whose first and second moments after n steps are closed forms; every statistic of 65536 realisations within 4 of its own
    standard errors (the standard error of a mean sqrt(var / N), of a variance var sqrt(2 / (N - 1)), of the covariance
    sqrt((var1 var2 + cov^2) / N): Gaussian sampling theory, nothing measured).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mc_ref as MC  # noqa: E402
import rollout_ref as R  # noqa: E402

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        got = tuple(int(v) for v in MC.philox4x32_10(ctr, key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])
    # the counter layout of words(): (r_lo, r_hi, step, j), key (seed_lo, seed_hi)
    w = MC.words(0x299f31d0a4093822, 0x85a308d3243f6a88, 1, 0x13198a2e, 1, 4)
    assert w.shape == (1, 1, 2, 4) and w.dtype == np.uint32
    assert tuple(int(v) for v in MC.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 1), (0xa4093822, 0x299f31d0))) == tuple(int(v) for v in w[0, 0, 1])
    assert MC.words(0xa4093822 | (0x299f31d0 << 32), 0x243f6a88 | (0x85a308d3 << 32), 1, 0x13198a2e, 1, 2).shape == (1, 1, 1, 4)


def test_uniforms_and_normals_of_the_words():
    """u1 in (0, 1], u2 in [0, 1): all-zero words give u1 = 2^-53 (the largest radius, finite), all-one words u1 = 1 (radius 0)."""
    z = MC.normals_of(np.zeros((1, 4), dtype=np.uint32), 2)
    assert np.isfinite(z).all() and z[1] == 0.0 and abs(z[0] - np.sqrt(-2 * np.log(2.0 ** -53))) < 1e-12
    z = MC.normals_of(np.full((1, 4), 0xffffffff, dtype=np.uint32), 2)
    assert np.array_equal(z, [0.0, -0.0]) or np.array_equal(np.abs(z), [0.0, 0.0])
    n = MC.normals(7, 0, 4096, 0, 8, 3)
    assert n.shape == (4096, 8, 3) and abs(n.mean()) < 4 / np.sqrt(n.size) and abs(n.var() - 1) < 4 * np.sqrt(2.0 / n.size)
    # an odd nd drops the second normal of the last pair; nd = 3 and nd = 4 share their first three
    assert np.array_equal(n, MC.normals(7, 0, 4096, 0, 8, 4)[..., :3])
    # a step's normals do not depend on how the steps are cut
    assert np.array_equal(n[:, 3:5], MC.normals(7, 0, 4096, 3, 2, 3)) and np.array_equal(n[100:200], MC.normals(7, 100, 100, 0, 8, 3))


def small_case():
    """Double integrator on 21^2 nodes of [-1, 1]^2, six shrinking discs, 12 states (one off the grid, one in the target)."""
    from oracle import hj_oracle as O
    og = O.Grid([-1, -1], [1, 1], [21, 21], [])
    xs = np.meshgrid(*[np.asarray(v).ravel() for v in og.vs], indexing='ij')
    r = np.sqrt(xs[0] ** 2 + xs[1] ** 2) + 0.1 * np.sin(2 * xs[0]) * np.cos(xs[1])
    data = np.stack([r - 0.7 + 0.1 * k for k in range(6)])
    tau = np.linspace(0, 0.5, 6)
    lat = np.linspace(-0.5, 0.5, 3)
    x0 = np.array([[a, b] for a in lat for b in lat] + [[1.5, 0.0], [0.9, 0.9], [0.05, 0.0]])
    return og, data, tau, x0


def test_zero_G_is_the_noise_free_rollout():
    og, data, tau, x0 = small_case()
    rtraj, rlen, rte, rstat, _ = R.rollout_ref(og, data, tau, "integrator", (1.0,), x0, 'min', 'min', 3, "ENO2")
    assert len(set(rlen.tolist())) >= 3 and set(rstat.tolist()) == {0, 1, 2}
    xi = np.random.default_rng(1).standard_normal((12, 3, 15, 2))
    out = MC.mc_ref(og, data, tau, "integrator", (1.0,), x0, np.zeros((2, 2)), 3, xi=xi, subSamples=3, scheme="ENO2")
    for k in range(3):
        assert np.array_equal(out["traj"][:, k], rtraj, equal_nan=True)
        assert np.array_equal(out["length"][:, k], rlen) and np.array_equal(out["status"][:, k], rstat)
        assert np.array_equal(out["t_earliest"][:, k], rte)
        last = rtraj[np.arange(12), :, rlen - 1]
        assert np.array_equal(out["final"][:, k], last, equal_nan=True)
        assert np.array_equal(out["value_end"][:, k], R._eval(og, data[-1], last), equal_nan=True)
    # with noise the generator decides, and a realisation is its (seed, index, step) alone: rows [4:9] with first = 4 R
    G = np.array([[0.02, 0.0], [0.01, 0.3]])
    full = MC.mc_ref(og, data, tau, "integrator", (1.0,), x0, G, 2, seed=5, subSamples=3, scheme="ENO2")
    part = MC.mc_ref(og, data, tau, "integrator", (1.0,), x0[4:9], G, 2, seed=5, first=8, subSamples=3, scheme="ENO2")
    assert all(np.array_equal(full[k][4:9], part[k], equal_nan=True) for k in full)
    assert not np.array_equal(full["final"][:9, 0], full["final"][:9, 1])
    # the clock policy never stops: full length, slice `it` at column `it`
    clock = MC.mc_ref(og, data, tau, "integrator", (1.0,), x0, G, 2, seed=5, policy='clock', subSamples=3, scheme="ENO2")
    assert (clock["length"] == 6).all() and (clock["t_earliest"] == np.array([0, 1, 2, 3, 4, -1])).all()
    assert set(clock["status"].ravel().tolist()) <= {R.EXHAUSTED, R.LEFT_GRID}
    tr = clock["traj"]
    v = np.stack([R._eval(og, data[-1], tr[:, k, :, c]) for k in range(2) for c in range(6)]).reshape(2, 6, 12)
    with np.errstate(invalid='ignore'):
        want_min = np.where(np.isnan(v).any(axis=1), np.nan, np.nanmin(np.where(np.isnan(v), np.inf, v), axis=1)).T
    assert np.array_equal(clock["value_min"], want_min, equal_nan=True) and np.array_equal(clock["value_end"], v[:, 5].T, equal_nan=True)


def moments_case():
    """The set-up of the discrete linear SDE, and its closed forms: (og, data, tau, x0, G, want) with want = dict of
    (value, standard error) for N = 65536."""
    from oracle import hj_oracle as O
    og = O.Grid([-2, -2], [2, 2], [41, 41], [])
    xs = np.meshgrid(*[np.asarray(v).ravel() for v in og.vs], indexing='ij')
    base = np.sqrt(xs[0] ** 2 + xs[1] ** 2 + 0.01) - 0.5
    tau = np.linspace(0, 0.5, 11)
    data = np.stack([base + 0.02 * k for k in range(11)])
    x0 = np.array([[0.3, -0.4]])
    g1, g2 = 0.05, 0.2
    n, N = 40, 65536
    h = (tau[1] - tau[0]) / 4
    var1 = g1 ** 2 * n * h + g2 ** 2 * h ** 3 * (n - 1) * n * (2 * n - 1) / 6
    var2 = g2 ** 2 * n * h
    cov = g2 ** 2 * h ** 2 * (n - 1) * n / 2
    want = dict(mean1=(0.3 + n * h * -0.4, np.sqrt(var1 / N)), mean2=(-0.4, np.sqrt(var2 / N)),
                var1=(var1, var1 * np.sqrt(2.0 / (N - 1))), var2=(var2, var2 * np.sqrt(2.0 / (N - 1))),
                cov=(cov, np.sqrt((var1 * var2 + cov ** 2) / N)))
    return og, data, tau, x0, np.diag([g1, g2]), want


def check_moments(final, status, want, who):
    """`final` (N, 2), `status` (N,): prints every statistic's distance in its own standard errors, then asserts 4."""
    assert (np.asarray(status) != R.LEFT_GRID).all(), "a realisation left the grid"
    c = np.cov(final.T)
    got = dict(mean1=final[:, 0].mean(), mean2=final[:, 1].mean(), var1=c[0, 0], var2=c[1, 1], cov=c[0, 1])
    off = {k: (got[k] - want[k][0]) / want[k][1] for k in want}
    print("%s: " % who + ", ".join("%s %+.2f se" % (k, off[k]) for k in sorted(off)) +
          "; variance ratios %.4f %.4f, covariance ratio %.4f" % (c[0, 0] / want["var1"][0], c[1, 1] / want["var2"][0], c[0, 1] / want["cov"][0]))
    for k in want:
        assert abs(off[k]) <= 4.0, (k, got[k], want[k], off[k])


def test_moments_of_the_discrete_linear_sde():
    og, data, tau, x0, G, want = moments_case()
    out = MC.mc_ref(og, data, tau, "integrator", (0.0,), x0, G, 65536, seed=20261021, policy='clock', subSamples=4, scheme="ENO2")
    assert (out["length"] == 11).all()
    check_moments(out["final"][0], out["status"][0], want, "restatement")
