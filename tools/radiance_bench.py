"""What a radiance query costs (R.RayCaster.radiance), in Msamples/s, on one GPU in one process.

The library's own calls (rtw_radiance_samples_device, rtw_radiance_resolve_device, rtw_render_device) on packed device
rays and preallocated outputs, on torch's current stream:
  (a) per scene of `--scenes` at `--width` x `--height`: one ray through the centre of every pixel (the lens centre,
      the shutter's opening time, built from the rtw_camera fields), `--samples` samples a ray, in pixel order and in a
      random order; the resolve (plain and finite) of that sample buffer; and `rtw_render_device` of the same world,
      size and sample count (the megakernel: SAH tree, LDS scene, cost-ordered queue; its camera rays are jittered),
      in the same process.  A sample of either is one path.
  (b) `--probe-rays` rays from random points inside the box of `--probe-scene` in random directions, `--probe-samples`
      samples each: few rays, many samples.
The constant under test is the loaded library's RTW_RAD_ITEMS (rtw_debug_radiance_items: the items a wave owns); the
sweep is this tool once per build (make variant V=rad64 DEFS=-DRTW_RAD_ITEMS=64, RTW_LIBRARY=.../librtw_rad64.so),
each in a fresh process, `--rates-only` for the builds that only differ in the constant.

Timing: device events around a window of back-to-back calls, as many as fill `--window-ms` (at least 2; counted per
call from one timed launch after the first warm-up, so a 0.6 ms resolve gets some 400 calls a window and a 160 ms
trace two), `--warmup` windows first, then `--runs` windows in `--rounds` alternating rounds over all the calls of
a scene; the table holds the calls a window, the median window, and the spread as (min, max) over all windows and as
(max - min) / median in per cent, per call.  No gate: a table.

python tools/radiance_bench.py [--out profiles/r24/radiance_bench.txt] [--append]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--max-depth", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--scenes", default="final_scene1,cornell_box,suzanne")
    ap.add_argument("--probe-scene", default="cornell_box")
    ap.add_argument("--probe-rays", type=int, default=4096)
    ap.add_argument("--probe-samples", type=int, default=1024)
    ap.add_argument("--rates-only", action="store_true", help="the radiance traces only: no resolve, shuffle or frame")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    import ctypes as C

    import torch

    import raytracinginaweekend_amd as R
    from raytracinginaweekend_amd import _native as N

    L = N.lib()
    items = L.rtw_debug_radiance_items()
    dev = torch.device("cuda", 0)
    size = R.Size2i(a.width, a.height)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream or 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def window(fn, launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(launches):
            fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) / launches

    def camera_rays(cam):
        v = lambda f: torch.tensor(list(f), dtype=torch.float32, device=dev)
        x = (torch.arange(a.width, dtype=torch.float32, device=dev) + 0.5) / a.width
        y = (torch.arange(a.height, dtype=torch.float32, device=dev) + 0.5) / a.height
        py, px = torch.meshgrid(y, x, indexing="ij")
        d = v(cam.upper_left_corner) + px.reshape(-1, 1) * v(cam.scaled_right) - py.reshape(-1, 1) * v(cam.scaled_up)
        d = d / d.norm(dim=1, keepdim=True)
        return v(cam.position).expand_as(d).contiguous(), d.contiguous()

    def measure(scene, calls):
        """calls: name -> (fn, samples a call).  Prints a row each; returns the medians (ms)."""
        times = {k: [] for k in calls}
        per = {}
        for k, (fn, _) in calls.items():
            window(fn, 2)  # (code objects, the frame's tuning)
            per[k] = max(2, int(math.ceil(a.window_ms / max(window(fn, 1), 1e-3))))
            for _ in range(a.warmup):
                window(fn, per[k])
        for _ in range(a.rounds):
            for k, (fn, _) in calls.items():
                times[k] += [window(fn, per[k]) for _ in range(a.runs)]
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for k, (_, n) in calls.items():
            rate = f"{n / med[k] / 1e3:10.1f}" if n else f"{'':10s}"
            lo, hi = min(times[k]), max(times[k])
            say(f"{scene:14s} {k:26s} {n:11d} {per[k]:6d} {med[k]:9.3f} {lo:9.3f} {hi:9.3f} {100 * (hi - lo) / med[k]:7.2f} {rate}")
        return med

    def trace_call(dworld, rays, samples, colors, seed=31):
        n = int(rays.shape[0])
        p = N.RadianceParams(0, 0, a.max_depth, samples, 0, 0, seed)
        pr, pc = C.c_void_p(rays.data_ptr()), C.c_void_p(colors.data_ptr())
        return lambda: N.check(L.rtw_radiance_samples_device(dworld._h, C.byref(p), pr, n, pc, sp)), n * samples

    say(f"radiance queries, RTW_RAD_ITEMS = {items} ({os.environ.get('RTW_LIBRARY', 'librtw.so')}): device tensors in and out, "
        f"max_depth {a.max_depth}; device events around windows of about {a.window_ms:.0f} ms, {a.warmup} warm-up windows, "
        f"{a.runs} windows x {a.rounds} alternating rounds; ms per call")
    say(f"{'world':14s} {'call':26s} {'samples':>11s} {'calls':>6s} {'median':>9s} {'min':>9s} {'max':>9s} {'spread%':>7s} {'Msamples/s':>10s}")
    for scene in [s for s in a.scenes.split(",") if s]:
        world = R.demo_world(scene)
        dworld = R.DeviceWorld(world, 0)
        c = R.RayCaster(dworld)
        o, d = camera_rays(world.raw.camera)
        tm = float(world.raw.camera.time0)
        rays = c._pack_device(o, d, tm, None)
        n = int(rays.shape[0])
        colors = torch.empty((n, a.samples, 3), dtype=torch.float32, device=dev)
        calls = {f"radiance x{a.samples} pixel order": trace_call(dworld, rays, a.samples, colors)}
        keep = [rays, colors]
        if not a.rates_only:
            gen = torch.Generator(device=dev)
            gen.manual_seed(24)
            shuffled = rays[torch.randperm(n, device=dev, generator=gen)].contiguous()
            mean = torch.empty((n, 3), dtype=torch.float32, device=dev)
            kept = torch.empty(n, dtype=torch.int32, device=dev)
            image = torch.empty((n, 3), dtype=torch.float32, device=dev)
            keep += [shuffled, mean, kept, image]
            calls[f"radiance x{a.samples} shuffled"] = trace_call(dworld, shuffled, a.samples, colors)
            pc, pm, pk = (C.c_void_p(t.data_ptr()) for t in (colors, mean, kept))
            q0 = N.RadianceParams(0, 0, a.max_depth, a.samples, 0, 0, 31)
            q1 = N.RadianceParams(N.RADIANCE_FINITE, 0, a.max_depth, a.samples, 0, 0, 31)
            calls["resolve"] = (lambda: N.check(L.rtw_radiance_resolve_device(C.byref(q0), pc, n, pm, None, sp)), 0)
            calls["resolve finite"] = (lambda: N.check(L.rtw_radiance_resolve_device(C.byref(q1), pc, n, pm, pk, sp)), 0)
            rp = R.render_params(size, a.samples, a.max_depth, seed=31)
            calls[f"rtw_render_device x{a.samples}"] = (lambda: dworld.render_into(rp, image.data_ptr(), stream.cuda_stream), n * a.samples)
        med = measure(scene, calls)
        if not a.rates_only:
            trace, frame = med[f"radiance x{a.samples} pixel order"], med[f"rtw_render_device x{a.samples}"]
            say(f"{scene:14s} radiance / frame, in Msamples/s: {frame / trace:.3f}; shuffled / pixel order: "
                f"{trace / med[f'radiance x{a.samples} shuffled']:.3f}; the resolve's share of trace + resolve: "
                f"{med['resolve'] / (trace + med['resolve']):.4f} (finite {med['resolve finite'] / (trace + med['resolve finite']):.4f})")
        del keep, calls
        dworld.release()
    if a.probe_rays > 0:
        world = R.demo_world(a.probe_scene)
        dworld = R.DeviceWorld(world, 0)
        c = R.RayCaster(dworld)
        root = world.raw.nodes[world.raw.root]
        gen = torch.Generator(device=dev)
        gen.manual_seed(25)
        lo = torch.tensor(list(root.min), dtype=torch.float32, device=dev)
        hi = torch.tensor(list(root.max), dtype=torch.float32, device=dev)
        o = lo + (hi - lo) * torch.rand((a.probe_rays, 3), device=dev, generator=gen)
        d = torch.randn((a.probe_rays, 3), device=dev, generator=gen)
        d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-6)
        rays = c._pack_device(o.contiguous(), d.contiguous(), float(world.raw.camera.time0), None)
        colors = torch.empty((a.probe_rays, a.probe_samples, 3), dtype=torch.float32, device=dev)
        measure(a.probe_scene, {f"probe {a.probe_rays} rays x{a.probe_samples}": trace_call(dworld, rays, a.probe_samples, colors)})
        dworld.release()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
