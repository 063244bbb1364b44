"""raytracinginaweekend_amd: MI355X-native replacement of the per-pixel render loop of
martingleich/RayTracingInAWeekend (src/lib/rendering.rs).

The product is librtw.so (HIP megakernel for gfx950 + host scene builder, C ABI in
include/rtw.h).  This package is its Python face, mirroring the reference's interface:
Camera.build()..., WorldBuilder / NodeBuilder, demo worlds, rendering.render(...).
"""
from . import image_io
from .aov import AovAccumulator, AovState, render_aov
from .cast import CastResult, RadianceResult, RayCaster, cast_rays, radiance_rays
from .denoise import Denoiser, denoise_host
from .progressive import (
    Accumulator,
    AccumState,
    render_adaptive,
    render_clamped,
    render_finite,
    render_progressive,
    render_to_noise,
    world_fingerprint,
)
from .rendering import (
    DeviceWorld,
    MultiDeviceWorld,
    RenderMode,
    Size2i,
    device_count,
    render,
    render_devices,
    render_params,
)
from .world import (
    DEMO_WORLDS,
    AssetSet,
    BackgroundColor,
    Camera,
    NodeBuilder,
    NodeRef,
    Rng,
    World,
    WorldBuilder,
    demo_world,
    load_obj_mesh,
)

__all__ = [
    "AccumState",
    "Accumulator",
    "AovAccumulator",
    "AovState",
    "AssetSet",
    "BackgroundColor",
    "Camera",
    "CastResult",
    "DEMO_WORLDS",
    "Denoiser",
    "DeviceWorld",
    "MultiDeviceWorld",
    "NodeBuilder",
    "NodeRef",
    "RadianceResult",
    "RayCaster",
    "RenderMode",
    "Rng",
    "Size2i",
    "World",
    "WorldBuilder",
    "cast_rays",
    "demo_world",
    "denoise_host",
    "device_count",
    "load_obj_mesh",
    "radiance_rays",
    "render",
    "render_aov",
    "render_devices",
    "render_adaptive",
    "render_clamped",
    "render_finite",
    "render_params",
    "render_progressive",
    "render_to_noise",
    "world_fingerprint",
]
