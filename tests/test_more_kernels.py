"""The six smoothing kernels beyond the first four -- WendlandQuinticC2_1D, WendlandQuinticC4, WendlandQuinticC4_1D,
WendlandQuinticC6, WendlandQuinticC6_1D, SuperGaussian -- on the host: the classes of pysph_amd/kernels.py against
tests/golden/kernels_more.npz (the reference's own Python classes, tests/golden/make_more_kernels_golden.py), the
reference's analytic values and moment identities (pysph/base/tests/test_kernel.py:362-515), and the mpmath
restatements of more_kernels.py pinned to the same file before they judge the device
(test_more_kernels_gpu.py)."""
import numpy as np
import pytest

from conftest import load_golden
from pysph_amd import kernels as K
import more_kernels as MK
import test_kernel_moments as KM


@pytest.mark.parametrize('kk,dim', MK.KIND_DIMS)
def test_host_classes_match_reference_fixture(kk, dim):
    """the assertion test_oracle_golden.py applies to the four host classes against kernels.npz: the boundary scalars
    equal, the vectorised helpers to rounding -- here for every helper"""
    g = load_golden('kernels_more.npz')
    name = MK.NAMES[kk]
    k = getattr(K, name)(dim=dim)
    key = '%s/%d/' % (name, dim)
    assert K.kernel_id(k) == kk
    assert k.fac == float(g[key + 'fac'])
    assert k.get_deltap() == float(g[key + 'deltap'])
    assert k.radius_scale == float(g[key + 'radius_scale'])
    h, r, xij = g[key + 'h'], g[key + 'r'], g[key + 'xij']
    assert np.count_nonzero(g[key + 'w']) > 16
    assert np.allclose(k.kernel(rij=r, h=h), g[key + 'w'], rtol=1e-12, atol=1e-30)
    assert np.allclose(k.dwdq(rij=r, h=h), g[key + 'dwdq'], rtol=1e-12, atol=1e-30)
    assert np.allclose(k.gradient_h(rij=r, h=h), g[key + 'gradh'], rtol=1e-11, atol=1e-12 * np.abs(g[key + 'gradh']).max())
    grad = k.gradient(xij=xij.T, rij=r, h=h)
    assert np.allclose(np.array(grad).T, g[key + 'grad'], rtol=1e-12, atol=1e-30)
    # get_correction: W(deltap h0, h0)
    h0 = 0.37
    w = K.get_correction(k, h0)
    ref, _ = MK.mp_kernel(kk, k.get_deltap(), dim)
    assert abs(w - float(ref) * k.fac / h0 ** dim) <= 1e-14 * abs(w)


def test_default_dimensions_are_the_references():
    """kernels.py:181,398,510,622,735,955"""
    assert [getattr(K, MK.NAMES[kk])().dim for kk in sorted(MK.NAMES)] == [1, 2, 1, 2, 1, 2]


@pytest.mark.parametrize('name,dim', [('WendlandQuinticC2_1D', 2), ('WendlandQuinticC2_1D', 3), ('WendlandQuinticC4', 1),
                                      ('WendlandQuinticC4_1D', 2), ('WendlandQuinticC4_1D', 3), ('WendlandQuinticC6', 1),
                                      ('WendlandQuinticC6_1D', 2), ('WendlandQuinticC6_1D', 3)])
def test_unsupported_dimension_raises(name, dim):
    with pytest.raises(ValueError) as e:
        getattr(K, name)(dim=dim)
    assert str(e.value) == '%s: Dim %d not supported' % (name, dim)


# test_kernel.py:366,389,411 / 453 / 478,485,492 / 501,508,515
W0 = {('SuperGaussian', 1): 1.5 / np.sqrt(np.pi), ('SuperGaussian', 2): 2.0 / np.pi, ('SuperGaussian', 3): 5.0 / (2.0 * np.pi ** 1.5),
      ('WendlandQuinticC2_1D', 1): 5.0 / 8.0,
      ('WendlandQuinticC4', 2): 9.0 / (4.0 * np.pi), ('WendlandQuinticC4', 3): 495.0 / (256.0 * np.pi),
      ('WendlandQuinticC4_1D', 1): 3.0 / 4.0,
      ('WendlandQuinticC6', 2): 78.0 / (28.0 * np.pi), ('WendlandQuinticC6', 3): 1365.0 / (512.0 * np.pi),
      ('WendlandQuinticC6_1D', 1): 55.0 / 64.0}


@pytest.mark.parametrize('name,dim', sorted(W0))
def test_kernel_at_origin_and_outside(name, dim):
    """check_kernel_at_origin (test_kernel.py:115-138): assertAlmostEqual's seven places"""
    k = getattr(K, name)(dim=dim)
    assert abs(float(k.kernel(rij=0.0, h=1.0)) - W0[(name, dim)]) < 0.5e-7
    assert float(k.kernel(rij=3.0, h=1.0)) == 0.0
    assert float(k.dwdq(rij=3.0, h=1.0)) == 0.0
    assert float(k.dwdq(rij=0.0, h=1.0)) == 0.0
    assert k.gradient(xij=(3.0, 0.0, 0.0), rij=3.0, h=1.0)[0] == 0.0


# (zeroth kernel moments: h = 1, h = 0.5, off-centre), first kernel moment, zeroth gradient moments, first gradient
# moment: TestCubicSpline1D, TestWendlandQuintic1D :455-469, TestSuperGaussian1D :368-382 over TestGaussian1D
PLACES_1D = {'WendlandQuinticC2_1D': ((8, 7, 7), 8, 8, 7), 'WendlandQuinticC4_1D': ((8, 8, 8), 8, 8, 8),
             'WendlandQuinticC6_1D': ((8, 8, 8), 8, 8, 8), 'SuperGaussian': ((3, 3, 3), 8, 8, 2)}


@pytest.mark.parametrize('name', sorted(PLACES_1D))
def test_1d_moments_by_quadrature(name):
    from scipy.integrate import quad
    k = getattr(K, name)(dim=1)
    kh = k.radius_scale
    p0, p1, pg0, pg1 = PLACES_1D[name]

    def tol(places):
        return 0.5 * 10.0 ** -places

    def q(f, a, b, pts):
        return quad(f, a, b, points=pts, limit=200)[0]

    for (a, b, h, xj), p in zip(((-kh, kh, 1.0, 0.0), (-kh, kh, 0.5, 0.0), (0.0, 2 * kh, 1.0, kh)), p0):
        pts = [xj + s * h for s in (-3, -2, -1, 0, 1, 2, 3) if a < xj + s * h < b]
        assert abs(q(lambda x: KM._w(k, x, xj, h), a, b, pts) - 1.0) < tol(p), (a, b, h, xj)
        assert abs(q(lambda x: KM._dw(k, x, xj, h), a, b, pts)) < tol(pg0)
    pts = [-2.0, -1.0, 0.0, 1.0, 2.0]
    assert abs(q(lambda x: x * KM._w(k, x, 0.0, 1.0), -kh, kh, pts)) < tol(p1)
    pts = [kh + s for s in (-2, -1, 0, 1, 2)]
    assert abs(q(lambda x: (x - kh) * KM._dw(k, x, kh, 1.0), 0.0, 2 * kh, pts) + 1.0) < tol(pg1)


# places of the lattice sums (zeroth moment, first gradient moment, off-axis gradient components): C4 / C6 2-D as
# TestCubicSpline2D, 3-D as TestGaussian3D, SuperGaussian :391-404 and :413-425
PLACES = {('WendlandQuinticC4', 2): (7, 6, 8), ('WendlandQuinticC6', 2): (7, 6, 8),
          ('WendlandQuinticC4', 3): (2, 2, 6), ('WendlandQuinticC6', 3): (2, 2, 6),
          ('SuperGaussian', 2): (2, 1, 8), ('SuperGaussian', 3): (2, 1, 6)}


@pytest.mark.parametrize('name,dim', sorted(PLACES))
def test_lattice_moments_host_kernels(name, dim):
    k = getattr(K, name)(dim=dim)
    x, y, z, vol = KM._lattice(dim)
    c = 0.5
    dx, dy, dz = x - c, y - c, (z - c if dim == 3 else z)
    r = np.sqrt(dx * dx + dy * dy + dz * dz)
    h = 0.15
    w = k.kernel(rij=r, h=h)
    p0, p1, p2 = PLACES[(name, dim)]
    assert abs(np.sum(w) * vol - 1.0) < 0.5 * 10.0 ** -p0
    assert abs(np.sum(dx * w) * vol) < 0.5e-7
    g = np.where(r > 1e-12, k.dwdq(rij=r, h=h) / h / np.maximum(r, 1e-300), 0.0)
    assert abs(np.sum(g * dx) * vol) < 0.5e-7
    assert abs(np.sum(dx * g * dx) * vol + 1.0) < 0.5 * 10.0 ** -p1
    assert abs(np.sum(dy * g * dx) * vol) < 0.5 * 10.0 ** -p2


@pytest.mark.parametrize('kk,dim', MK.KIND_DIMS)
def test_mpmath_restatements_reproduce_the_fixture(kk, dim):
    """more_kernels.mp_kernel / mp_kernel_all retrace tests/golden/kernels_more.npz (w, dwdq, the gradient and
    gradient_h of the reference's own classes in fp64) to the 2 ulp test_device_functions.py holds the first four to:
    at a working precision of 53 bits mpmath rounds every operation like IEEE double, so the reference's lines in the
    reference's order give the file's values rounding by rounding -- up to libm's exp against the correctly rounded
    one.  gradient_h subtracts two terms of opposite sign: its stored value is judged in ulps of the larger term."""
    import mpmath as mp
    g = load_golden('kernels_more.npz')
    key = '%s/%d/' % (MK.NAMES[kk], dim)
    h, r, xij, sigma = g[key + 'h'], g[key + 'r'], g[key + 'xij'], float(g[key + 'fac'])
    worst = {'w': 0.0, 'dwdq': 0.0, 'grad': 0.0, 'gradh': 0.0}
    inside = 0
    with mp.workprec(53):
        for i in range(h.size):
            w, dw, grad, gh = MK.mp_kernel_all(kk, r[i], h[i], sigma, dim, xij[i])
            inside += w != 0
            stored = [('w', g[key + 'w'][i], w), ('dwdq', g[key + 'dwdq'][i], dw), ('gradh', g[key + 'gradh'][i], gh)]
            stored += [('grad', g[key + 'grad'][i][c], grad[c]) for c in range(3)]
            for name, got, ref in stored:
                ref = float(ref)
                if ref == 0:
                    assert got == 0, (name, i, got)
                else:
                    scale = abs(ref)
                    if name == 'gradh':
                        scale = max(scale, abs(float(w)) * dim / h[i])
                    worst[name] = max(worst[name], abs(got - ref) / np.spacing(scale))
    print('%s dim %d: max ulp %s' % (MK.NAMES[kk], dim, ', '.join('%s %.2f' % kv for kv in sorted(worst.items()))))
    assert inside > 16
    assert max(worst.values()) <= 2, worst
