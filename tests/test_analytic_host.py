"""The oracle's estimator against closed-form f64 expectations (tests/analytic_scenes.py), on the CPU.

The parity tests compare kernel and oracle, which share include/rtw_scalar.h: a wrong sampler, pdf or coin
in the shared spec is invisible to them.  Here the oracle renders scenes whose per-pixel expectation is a
closed-form number, and the image mean must sit within 5 standard errors of it; the standard error comes from
the f64 single-sample variance (S2m: from the spread of 8 seeds), never from the image under test, and the
midpoint rule's own error (the change from n to 2 n) must stay below a quarter of it.

Set RTW_ANALYTIC_REPORT to a file name to have every figure appended to it."""
import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from tests import analytic_scenes as A

W = H = 48
SPP = 4096
THREADS = 16


def oracle_image(world, w, h, spp, seed=A.SEED):
    return O.render(world, R.render_params(R.Size2i(w, h), spp, A.MAX_DEPTH, seed=seed), O.RNG_CTR, THREADS)


def test_s1_weight_is_exactly_one():
    """S1: spdf / p has identical operands, so every sample is f32(albedo background) bit for bit -- or 0 where the
    algorithm as written traps the bounce inside the sphere (analytic_scenes.s1_trap_probability); each pixel short
    of the constant is traced to samples whose bounce, with two levels of depth, hit the sphere again."""
    world, (w, h), expect = A.s1_weight()
    spp = 256
    img = oracle_image(world, w, h, spp)
    trapped = A.assert_s1(img, world, w, h, spp)
    e = expect(world, w, h)
    scale = e.scale.astype(np.float32)
    p2 = R.render_params(R.Size2i(w, h), spp, 2, seed=A.SEED)
    found = 0
    for pix in np.flatnonzero((img != scale).any(axis=1)):
        col = np.array([O.sample_color(world, p2, int(pix % w), int(pix // w), s) for s in range(spp)])
        zero = ~col.any(axis=1)
        assert (col[~zero] == scale).all()
        assert img[pix, 0] == np.float32(scale[0] * np.float32(spp - zero.sum()) / np.float32(spp))
        found += int(zero.sum())
    assert found == trapped
    A.report(f"cpu S1 {w}x{h}x{spp} samples={w * h * spp} every sample albedo*background={e.scale.tolist()} bit for "
             f"bit, but {trapped} trapped (bound {A.s1_trap_probability(world) * w * h * spp:.1f})")


@pytest.mark.parametrize("name", A.BERNOULLI)
def test_image_mean(name):
    A.check_image_mean(oracle_image, name, W, H, SPP, "cpu")


def test_light_mixture_mean():
    A.check_mixture_mean(oracle_image, W, H, 1024, "cpu")


def test_lens_disc_columns():
    A.check_lens_columns(oracle_image, W, H, SPP, "cpu")


def test_dispersion_over_pixels():
    A.check_dispersion(oracle_image, 64, 64, 256, "cpu")


def test_dispersion_over_sample_index():
    """The same statistic over the sample index: the mean over one 8 x 8 block of pixels of sample s, for each s
    (streams shared between the block's pixels would inflate it 64-fold)."""
    world, (w, h), expect = A.s2_cosine_lobe(64, 64)
    spp = 256
    e = expect(world, w, h)
    p = R.render_params(R.Size2i(w, h), spp, A.MAX_DEPTH, seed=A.SEED)
    bx, by = 24, 32
    block = np.array([[[O.sample_color(world, p, bx + i, by + j, s) for s in range(spp)] for i in range(8)]
                      for j in range(8)], np.float64) / e.scale  # (8, 8, spp, 3)
    assert np.isin(block, (0.0, 1.0)).all()
    # the block's samples are the oracle's image
    img = A.normalised(oracle_image(world, w, h, spp), e, w, h)
    assert (block[..., 0].sum(axis=2) == img[by:by + 8, bx:bx + 8, 0] * spp).all()
    f = e.mean[by:by + 8, bx:bx + 8]
    m_s = block[..., 0].mean(axis=(0, 1))
    chi2 = float(((m_s - f.mean()) ** 2 / ((f * (1 - f)).sum() / 64.0**2)).sum())
    bound = 5.0 * np.sqrt(2.0 * spp)
    A.report(f"cpu S2 dispersion over sample index, block ({bx},{by}) 8x8x{spp}: chi2={chi2:.1f} n={spp} "
             f"bound=+-{bound:.1f}")
    assert abs(chi2 - spp) <= bound
