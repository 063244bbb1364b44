"""What a path does at a hit, on the device: shade() and the radiance kernels' bookkeeping against
tests/path_ref.py's f64 stepper, under the constants tests/test_path_host.py measured on the oracle, nothing added.

No device entry point returns vertices; the device is reached through R.RayCaster.radiance(per_sample=True), whose
sample k of ray i runs ray_color from the stream (seed, i, k):

  * leg d of the host test through the device: the vertex rays as query rays, 4 samples, max_depth 2 (sky copies) and 3
    (detector copies) against the stepper's one-bounce prediction -- and bit for bit against rtw_oracle_ray_color, so a
    tolerance failure that the host leg passes can only be a kernel bug;
  * the camera rays of every world at max_depth 1, 2, 3 and 6: bit for bit the oracle's colour and the numpy-f32 replay
    of leg c (tests/path_ref.replay) -- the bookkeeping quirks on the device against the replay, not only the oracle;
  * one frame of every detector world, 48 x 27, 4 spp, depth 6, bit for bit against the oracle's: the megakernel's
    shade() instantiation (and the first-bounce fill where the world takes it) on these materials."""
import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from tests import path_check as Pc
from tests import path_ref as P
from tests import path_worlds as PW
from tests.parity import assert_bit_identical

pytestmark = pytest.mark.gpu

BOTH = [(n, c) for n in PW.NAMES for c in PW.COPIES]
IDS = [f"{n} {c}" for n, c in BOTH]
CAMERA_SAMPLES = 2
_casters = {}


def caster(name, copy):
    """One upload per world for the whole module."""
    if (name, copy) not in _casters:
        _casters[name, copy] = R.RayCaster(PW.world(name, copy))
    return _casters[name, copy]


@pytest.mark.parametrize("name, copy", BOTH, ids=IDS)
def test_one_bounce_on_the_device(name, copy):
    depth = Pc.BOUNCE_DEPTH[copy]
    rays = Pc.query_rays(name, copy)
    res = caster(name, copy).radiance(rays[:, 0:3], rays[:, 4:7], rays[:, 3], samples=Pc.QUERY_SAMPLES, max_depth=depth,
                                      seed=Pc.SEED, first_ray=0, first_sample=0, per_sample=True)
    assert res.samples.dtype == np.float32 and res.samples.shape == (len(rays), Pc.QUERY_SAMPLES, 3)
    worst, left = Pc.compare_one_bounce(name, copy, res.samples, f"device, {name} {copy}, max_depth {depth}")
    print(f"device {name} {copy}: {len(rays)} query rays x {Pc.QUERY_SAMPLES}, left out {100 * left:.2f} %, "
          f"worst (U S) {worst:.3f} (allowed {P.K['colour']})")
    assert left <= Pc.MAX_LEFT_OUT
    assert_bit_identical(res.samples, Pc.oracle_query_samples(name, copy, depth), f"{name} {copy}: samples against the oracle")


@pytest.mark.parametrize("name, copy", BOTH, ids=IDS)
def test_camera_rays_on_the_device(name, copy):
    world = PW.world(name, copy)
    (o, d, t, _), _, _, _ = Pc.camera_paths(name, copy)
    rep = lambda a: np.repeat(a, CAMERA_SAMPLES, axis=0)
    streams = Pc.query_streams(len(o), samples=CAMERA_SAMPLES)  # the radiance queries' streams, not the frame's
    vertices, counts, _, _ = O.paths(world, rep(o), rep(d), rep(t), streams, Pc.DEPTH)
    c = caster(name, copy)
    for max_depth in (1, 2, 3, 6):
        res = c.radiance(o, d, t, samples=CAMERA_SAMPLES, max_depth=max_depth, seed=Pc.SEED, per_sample=True)
        got = res.samples.reshape(-1, 3)
        colors, _ = O.ray_colors(world, rep(o), rep(d), rep(t), streams, max_depth)
        assert_bit_identical(got, colors, f"{name} {copy}, max_depth {max_depth}: samples against the oracle")
        assert_bit_identical(got, P.replay(vertices, counts, max_depth), f"{name} {copy}, max_depth {max_depth}: against the replay")
        if max_depth == 1:  # a hit is black, a miss the background
            assert (got[vertices[:, 0]["hit"] == 1] == 0).all()
    assert (counts >= 3).sum() >= 200


@pytest.mark.parametrize("name", PW.NAMES)
def test_frames_of_the_detector_worlds(name):
    import torch

    world = PW.world(name, "detector")
    p = R.render_params(R.Size2i(48, 27), 4, Pc.DEPTH, seed=Pc.SEED)
    dw = R.DeviceWorld(world, 0)
    try:
        out = torch.zeros(p.width * p.height * 3, dtype=torch.float32, device="cuda:0")
        dw.render_into(p, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        print(f"{name}: {dw.kernel_variant()['name']}")
        assert_bit_identical(out.cpu().numpy().reshape(-1, 3), O.render(world, p), f"{name}: a 48 x 27 frame against the oracle")
    finally:
        dw.release()
