"""What a ray query costs (R.RayCaster), in Mrays/s, on one GPU in one process.

Per scene of `--scenes` at `--width` x `--height`, every ray set as packed rtw_ray records on the device, closest hit
(rtw_cast_device) and occlusion (rtw_occluded_device), one launch a call:
  camera    the frame's camera rays in pixel order: one ray through every pixel (no jitter, the lens centre, the
            shutter's opening time), built from the rtw_camera fields
  shuffled  the same rays in a random order
  bounce    one ray from every camera hit: the hit position, a direction drawn around the hit normal (normal + a
            random unit vector: Lambertian-like), the camera ray's time
The comparator is `AovAccumulator.add(1)` (rtw_aov_add, called as directly as the queries) on the same world and size
with RTW_PRIMARY_LISTS=0: the same walk on the frame's (jittered) camera rays, minus the 32 B read and 48 B written
per ray -- and plus its plane reads and stores, 28 B + 28 B per ray.  Its rate counts one ray per pixel.

Timing: device events around `--launches` back-to-back launches, `--warmup` windows first, then `--runs` windows in
`--rounds` alternating rounds over all the calls of a scene; the table holds the median window, and the spread as
(min, max) over all windows, per launch.  No gate: a table.

python tools/cast_bench.py [--out profiles/r23/cast_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--scenes", default="final_scene1,cornell_box,suzanne")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["RTW_PRIMARY_LISTS"] = "0"  # the comparator walks every camera ray, as the queries do
    import ctypes as C

    import torch

    import raytracinginaweekend_amd as R
    from raytracinginaweekend_amd import _native as N

    L = N.lib()
    p = N.CastParams(0, 0.001, 31, 0, 0)
    dev = torch.device("cuda", 0)
    size = R.Size2i(a.width, a.height)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream or 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def window(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(a.launches):
            fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) / a.launches

    def camera_rays(cam):
        v = lambda f: torch.tensor(list(f), dtype=torch.float32, device=dev)
        x = torch.arange(a.width, dtype=torch.float32, device=dev) / (a.width - 1)
        y = torch.arange(a.height, dtype=torch.float32, device=dev) / (a.height - 1)
        py, px = torch.meshgrid(y, x, indexing="ij")
        d = v(cam.upper_left_corner) + px.reshape(-1, 1) * v(cam.scaled_right) - py.reshape(-1, 1) * v(cam.scaled_up)
        d = d / d.norm(dim=1, keepdim=True)
        return v(cam.position).expand_as(d).contiguous(), d.contiguous()

    say(f"ray queries at {a.width}x{a.height} ({a.width * a.height} rays a set), device tensors in and out; device events around "
        f"{a.launches} launches, {a.warmup} warm-up windows, {a.runs} windows x {a.rounds} alternating rounds; ms per launch")
    say(f"{'world':14s} {'call':22s} {'rays':>9s} {'median':>8s} {'min':>8s} {'max':>8s} {'Mrays/s':>9s} {'/ AOV add':>9s}")
    for scene in [s for s in a.scenes.split(",") if s]:
        world = R.demo_world(scene)
        dworld = R.DeviceWorld(world, 0)
        c = R.RayCaster(dworld)
        o, d = camera_rays(world.raw.camera)
        tm = float(world.raw.camera.time0)
        gen = torch.Generator(device=dev)
        gen.manual_seed(23)
        perm = torch.randperm(o.shape[0], device=dev, generator=gen)
        first = c.cast(o, d, tm)
        h = first.hit
        rnd = torch.randn((int(h.sum()), 3), device=dev, generator=gen)
        bd = first.normal[h] + rnd / rnd.norm(dim=1, keepdim=True)
        bo = first.position[h].contiguous()
        bd = (bd / bd.norm(dim=1, keepdim=True).clamp_min(1e-6)).contiguous()
        sets = {"camera": (o, d), "shuffled": (o[perm].contiguous(), d[perm].contiguous()), "bounce": (bo, bd)}
        aov = R.AovAccumulator(dworld, size, seed=31)
        # (the library's own call on the prefetched stream, like the casts below: no Python wrapper in the window)
        calls = {"AovAccumulator.add(1)": (lambda: N.check(L.rtw_aov_add(aov._h, 1, sp)), o.shape[0])}
        keep = []  # the packed rays and the outputs: the calls below are the library's own, one launch each
        for name, (ro, rd) in sets.items():
            rays = c._pack_device(ro, rd, tm, None)
            n = int(rays.shape[0])
            hits = torch.empty((n, 12), dtype=torch.float32, device=dev)
            out = torch.empty(n, dtype=torch.uint8, device=dev)
            keep.append((rays, hits, out))
            pr, ph, po = (C.c_void_p(t.data_ptr()) for t in (rays, hits, out))
            calls[f"cast {name}"] = (lambda pr=pr, ph=ph, n=n: N.check(L.rtw_cast_device(dworld._h, C.byref(p), pr, n, ph, None, sp)), n)
            calls[f"occluded {name}"] = (lambda pr=pr, po=po, n=n: N.check(L.rtw_occluded_device(dworld._h, C.byref(p), pr, n, po, sp)), n)
        times = {k: [] for k in calls}
        for k, (fn, _) in calls.items():
            for _ in range(a.warmup):
                window(fn)
        for _ in range(a.rounds):
            for k, (fn, _) in calls.items():
                times[k] += [window(fn) for _ in range(a.runs)]
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        base = calls["AovAccumulator.add(1)"][1] / med["AovAccumulator.add(1)"]
        for k, (_, n) in calls.items():
            rate = n / med[k]  # rays per ms
            say(f"{scene:14s} {k:22s} {n:9d} {med[k]:8.3f} {min(times[k]):8.3f} {max(times[k]):8.3f} {rate / 1e3:9.1f} {rate / base:9.2f}")
        say(f"{scene:14s} camera hits {int(h.sum())} of {o.shape[0]}")
        aov.release()
        dworld.release()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
