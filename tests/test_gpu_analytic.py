"""The render kernels against closed-form f64 expectations (tests/analytic_scenes.py), through the public R.render.

Two axes: each scene, a world shape of its own (one- and two-leaf worlds, a camera inside the lens blur, a volume
alone), is bit-identical to the oracle at 32 x 32 x 16; and at 2.7e8 samples the image mean sits within 5 standard
errors (about 1e-4 relative) of the closed form, under the same rules as tests/test_analytic_host.py.  A failure
here that the oracle's smaller run passes is a kernel bug.

Set RTW_ANALYTIC_REPORT to a file name to have every figure appended to it."""
import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from tests import analytic_scenes as A
from tests.parity import assert_bit_identical

pytestmark = pytest.mark.gpu

W = H = 256
SPP = 4096


def gpu_image(world, w, h, spp, seed=A.SEED):
    return R.render(R.Size2i(w, h), 1, spp, A.MAX_DEPTH, world, seed=seed, device=0)


def oracle_image(world, w, h, spp, seed=A.SEED):
    return O.render(world, R.render_params(R.Size2i(w, h), spp, A.MAX_DEPTH, seed=seed), O.RNG_CTR, 16)


def kernel_name(world, w, h, spp, want) -> str:
    """The kernel a resident copy of the world renders this frame with (kernel_variant()); its image is `want` too."""
    import torch

    dw = R.DeviceWorld(world, 0)
    try:
        out = torch.empty(w * h * 3, dtype=torch.float32, device="cuda:0")
        dw.render_into(R.render_params(R.Size2i(w, h), spp, A.MAX_DEPTH, seed=A.SEED), out.data_ptr(), 0)
        torch.cuda.synchronize()
        assert_bit_identical(out.cpu().numpy().reshape(-1, 3), want, "resident world")
        return dw.kernel_variant()["name"]
    finally:
        dw.release()


@pytest.mark.parametrize("name", list(A.SCENES))
def test_bit_identical_to_the_oracle(name):
    world, (w, h), _ = A.SCENES[name](32, 32)
    gpu, ref = gpu_image(world, w, h, 16), oracle_image(world, w, h, 16)
    assert_bit_identical(gpu, ref, name)
    A.report(f"gpu {name} {w}x{h}x16 bit-identical to the oracle; kernel {kernel_name(world, w, h, 16, ref)}")


def test_s1_weight_is_exactly_one():
    """Every sample f32(albedo background) bit for bit, or trapped and 0 (analytic_scenes.assert_s1), and the very
    image of the oracle."""
    world, (w, h), _ = A.s1_weight(64, 64)
    gpu = gpu_image(world, w, h, SPP)
    trapped = A.assert_s1(gpu, world, w, h, SPP)
    assert_bit_identical(gpu, oracle_image(world, w, h, SPP), "S1")
    A.report(f"gpu S1 {w}x{h}x{SPP} samples={w * h * SPP} every sample albedo*background bit for bit, but {trapped} "
             f"trapped (bound {A.s1_trap_probability(world) * w * h * SPP:.1f}); the oracle's image")


@pytest.mark.parametrize("name", A.BERNOULLI)
def test_image_mean(name):
    A.check_image_mean(gpu_image, name, W, H, SPP, "gpu")


def test_light_mixture_mean():
    A.check_mixture_mean(gpu_image, W, H, 1024, "gpu")


def test_lens_disc_columns():
    A.check_lens_columns(gpu_image, W, H, SPP, "gpu")


def test_dispersion_over_pixels():
    A.check_dispersion(gpu_image, W, H, 256, "gpu")
