"""Ray queries without a GPU (rtw_cast_*, rtw_occluded_*, include/rtw.h): the records' layout, every
refusal that needs no device -- parameters are checked before the world, so a bad parameter with a NULL world names
the parameter and good parameters with a NULL world name the world -- and the Python argument errors."""
import ctypes as C

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd import cast as RC

f32 = np.float32


def test_record_layout():
    assert C.sizeof(N.Ray) == 32 and C.sizeof(N.Hit) == 48
    assert [(n, getattr(N.Ray, n).offset) for n, _ in N.Ray._fields_] == [("origin", 0), ("time", 12), ("direction", 16), ("t_end", 28)]
    assert [(n, getattr(N.Hit, n).offset) for n, _ in N.Hit._fields_] == [
        ("t", 0), ("leaf", 4), ("position", 8), ("normal", 20), ("uv", 32), ("front_face", 40), ("material", 44)]
    assert C.sizeof(N.CastParams) == 24
    assert [(n, getattr(N.CastParams, n).offset) for n, _ in N.CastParams._fields_] == [
        ("flags", 0), ("t_start", 4), ("seed", 8), ("stream", 16), ("reserved0", 20)]
    assert N.CAST_ALBEDO == 1
    assert RC.RAY_WORDS * 4 == 32 and RC.HIT_WORDS * 4 == 48


def test_version_is_unchanged():
    assert N.lib().rtw_version() == 2 == N.ABI_VERSION


class Buffers:
    """Host arrays of 4 rays, 16-byte aligned (the device calls check the alignment before the world)."""

    def __init__(self):
        self.raw = np.zeros(4 * 8 + 4 * 12 + 4 * 3 + 16 + 8, f32)
        skip = (-self.raw.ctypes.data % 16) // 4
        a = self.raw[skip:]
        self.rays, self.hits, self.albedo, self.out = a[:32], a[32:80], a[80:92], a[92:108].view(np.uint8)
        assert self.rays.ctypes.data % 16 == 0 and self.hits.ctypes.data % 16 == 0
        self.before = self.raw.copy()

    def untouched(self):
        return np.array_equal(self.raw.view(np.uint32), self.before.view(np.uint32))


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def params(**kw):
    p = N.CastParams(0, 0.001, 1, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def refused(rc, match):
    assert rc == N.RTW_ERR_INVALID_ARGUMENT, rc
    msg = N.lib().rtw_last_error().decode()
    assert match in msg, msg


# (what is wrong, params, n, rays?, out?, albedo?, the message's words) for the closest-hit calls
CAST_REFUSALS = [
    ("flags", dict(flags=2), 4, True, True, False, "rtw_cast_params.flags"),
    ("flags high", dict(flags=0x80000001), 4, True, True, True, "rtw_cast_params.flags"),
    ("reserved0", dict(reserved0=1), 4, True, True, False, "rtw_cast_params.reserved0"),
    ("t_start nan", dict(t_start=float("nan")), 4, True, True, False, "rtw_cast_params.t_start"),
    ("t_start inf", dict(t_start=float("inf")), 4, True, True, False, "rtw_cast_params.t_start"),
    ("t_start -inf", dict(t_start=float("-inf")), 4, True, True, False, "rtw_cast_params.t_start"),
    ("n < 0", {}, -1, True, True, False, "n must be within"),
    ("n > 2^31 - 1", {}, 1 << 31, True, True, False, "n must be within"),
    ("rays", {}, 4, False, True, False, "null rays"),
    ("hits", {}, 4, True, False, False, "null hits"),
    ("albedo missing", dict(flags=1), 4, True, True, False, "null albedo"),
    ("albedo unasked", {}, 4, True, True, True, "albedo given"),
]


@pytest.mark.parametrize("device_call", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("case", CAST_REFUSALS, ids=[c[0] for c in CAST_REFUSALS])
def test_cast_refusals_name_the_parameter(case, device_call):
    _, kw, n, rays, out, albedo, match = case
    L, b, p = N.lib(), Buffers(), params(**kw)
    args = [None, C.byref(p), ptr(b.rays if rays else None), n, ptr(b.hits if out else None), ptr(b.albedo if albedo else None)]
    refused(L.rtw_cast_device(*args, None) if device_call else L.rtw_cast(*args), match)
    assert b.untouched()


OCCLUDED_REFUSALS = [
    ("flags", dict(flags=1), 4, True, True, "rtw_cast_params.flags"),  # (the occlusion calls know no flag)
    ("reserved0", dict(reserved0=7), 4, True, True, "rtw_cast_params.reserved0"),
    ("t_start nan", dict(t_start=float("nan")), 4, True, True, "rtw_cast_params.t_start"),
    ("n < 0", {}, -5, True, True, "n must be within"),
    ("n > 2^31 - 1", {}, 1 << 40, True, True, "n must be within"),
    ("rays", {}, 4, False, True, "null rays"),
    ("out", {}, 4, True, False, "null out"),
]


@pytest.mark.parametrize("device_call", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("case", OCCLUDED_REFUSALS, ids=[c[0] for c in OCCLUDED_REFUSALS])
def test_occluded_refusals_name_the_parameter(case, device_call):
    _, kw, n, rays, out, match = case
    L, b, p = N.lib(), Buffers(), params(**kw)
    args = [None, C.byref(p), ptr(b.rays if rays else None), n, ptr(b.out if out else None)]
    refused(L.rtw_occluded_device(*args, None) if device_call else L.rtw_occluded(*args), match)
    assert b.untouched()


def test_null_params():
    L, b = N.lib(), Buffers()
    refused(L.rtw_cast_device(None, None, ptr(b.rays), 4, ptr(b.hits), None, None), "null params")
    refused(L.rtw_occluded(None, None, ptr(b.rays), 4, ptr(b.out)), "null params")


def test_misaligned_device_buffers():
    L, b, p = N.lib(), Buffers(), params()
    refused(L.rtw_cast_device(None, C.byref(p), C.c_void_p(b.rays.ctypes.data + 4), 1, ptr(b.hits), None, None), "rays must be 16-byte")
    refused(L.rtw_cast_device(None, C.byref(p), ptr(b.rays), 1, C.c_void_p(b.hits.ctypes.data + 8), None, None), "hits must be 16-byte")
    refused(L.rtw_occluded_device(None, C.byref(p), C.c_void_p(b.rays.ctypes.data + 4), 1, ptr(b.out), None), "rays must be 16-byte")
    # host arrays are staged: any alignment passes on to the next check, the world
    refused(L.rtw_cast(None, C.byref(p), C.c_void_p(b.rays.ctypes.data + 4), 1, C.c_void_p(b.hits.ctypes.data + 4), None), "null world")


@pytest.mark.parametrize("n", [0, 4, (1 << 31) - 1])
def test_good_parameters_name_the_world(n):
    L, b = N.lib(), Buffers()
    p = params(flags=1, t_start=-2.5, seed=(1 << 64) - 1, stream=(1 << 32) - 1)
    refused(L.rtw_cast_device(None, C.byref(p), ptr(b.rays), n, ptr(b.hits), ptr(b.albedo), None), "null world")
    refused(L.rtw_cast(None, C.byref(p), ptr(b.rays), n, ptr(b.hits), ptr(b.albedo)), "null world")
    p.flags = 0
    refused(L.rtw_occluded_device(None, C.byref(p), ptr(b.rays), n, ptr(b.out), None), "null world")
    refused(L.rtw_occluded(None, C.byref(p), ptr(b.rays), n, ptr(b.out)), "null world")
    assert b.untouched()


# ---- the Python arguments ----------------------------------------------------------------------------------------------
def test_pack_rays_broadcasts():
    o = np.arange(15, dtype=np.float64).reshape(5, 3)
    rays = RC.pack_rays(o, (0, 0, -1), 0.5, [1, 2, 3, 4, 5])
    assert rays.dtype == f32 and rays.shape == (5, 8)
    assert np.array_equal(rays[:, :3], o.astype(f32)) and (rays[:, 3] == 0.5).all()
    assert (rays[:, 4:7] == [0, 0, -1]).all() and list(rays[:, 7]) == [1, 2, 3, 4, 5]
    rays = RC.pack_rays((1, 2, 3), np.ones((2, 3), f32))
    assert rays.shape == (2, 8) and (rays[:, 3] == 0).all() and np.isinf(rays[:, 7]).all()
    assert RC.pack_rays(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 8)
    assert RC.pack_rays(np.zeros((0, 3)), (0, 0, 1), 0.0, np.inf).shape == (0, 8)


BAD_RAYS = [
    ("origins", dict(origins=np.zeros((4, 2)))),
    ("origins", dict(origins=np.zeros((2, 4, 3)))),
    ("origins", dict(origins=np.zeros(4))),
    ("origins", dict(origins=np.zeros((4, 3), np.complex64))),
    ("directions", dict(directions=np.zeros((3, 3)))),  # 3 rays beside 4
    ("directions", dict(directions=[["a", "b", "c"]])),
    ("directions", dict(directions=np.zeros((4, 3, 1)))),
    ("times", dict(times=np.zeros((4, 1)))),
    ("times", dict(times=np.zeros(5))),
    ("times", dict(times="now")),
    ("t_end", dict(t_end=np.zeros(3))),
    ("t_end", dict(t_end=np.zeros((2, 2)))),
    ("t_end", dict(t_end=1j)),
]


@pytest.mark.parametrize("name, bad", BAD_RAYS, ids=[f"{n}{i}" for i, (n, _) in enumerate(BAD_RAYS)])
def test_ray_arguments_are_named(name, bad):
    good = dict(origins=np.zeros((4, 3), f32), directions=np.ones((4, 3), f32), times=None, t_end=None)
    good.update(bad)
    with pytest.raises(ValueError, match=f"^{name}:"):
        RC.pack_rays(**good)


@pytest.mark.parametrize("name, kw", [("t_start", dict(t_start=float("nan"))), ("t_start", dict(t_start=float("inf"))),
                                      ("t_start", dict(t_start="soon")), ("seed", dict(seed=-1)), ("seed", dict(seed=1 << 64)),
                                      ("seed", dict(seed=1.5)), ("stream", dict(stream=-1)), ("stream", dict(stream=1 << 32)),
                                      ("stream", dict(stream=True))])
def test_call_arguments_are_named(name, kw):
    args = dict(t_start=0.001, seed=1, stream=0, albedo=False)
    args.update(kw)
    with pytest.raises(ValueError, match=f"^{name}:"):
        RC._params(**args)


def test_params_are_the_arguments():
    p = RC._params(0.25, (1 << 64) - 1, 3, True)
    assert (p.flags, p.t_start, p.seed, p.stream, p.reserved0) == (1, 0.25, (1 << 64) - 1, 3, 0)
    assert RC._params(0, np.int64(5), np.uint32(2), False).flags == 0


def test_the_package_exports_the_caster():
    assert R.RayCaster is RC.RayCaster and R.cast_rays is RC.cast_rays and R.CastResult is RC.CastResult
    assert {"RayCaster", "cast_rays", "CastResult"} <= set(R.__all__)
