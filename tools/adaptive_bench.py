"""What adaptive sampling costs and saves, on one GPU in one process.

Device events around work that ends in a synchronise; the variants alternate `--rounds` times after a warm-up of
each; every variant renders through its own resident world (a world keeps one learned tile order).

1. Overhead while nothing stops: adds of `--add` samples up to `--spp` on a plain moments accumulator (the
   yardstick, the parent's code path) against the same adds on an adaptive accumulator with an adapt(target 0)
   after each -- no tile stops, so the launches are the same and the difference is the tile test and its
   synchronise.  The ratio is reported beside the yardstick's own spread; the adapt call is also timed alone
   (host clock around the synchronous call on an idle device, and device events around it).
2. Equal-target cost: render_to_noise and render_adaptive to the same target, taken from a uniform
   `--target-spp` frame's noise(), capped at `--max-samples`: ms, samples rendered, and noise() of both results.
   (The uniform loop stops when the frame's mean error meets the target, the adaptive one stops each tile when
   its worst pixel does: at the same number the adaptive frame is the stricter one.  So a third run takes the
   uniform loop to the noise() the adaptive frame reached, capped at twice `--max-samples`.)

python tools/adaptive_bench.py [--out profiles/r09/adaptive_bench.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--add", type=int, default=64)
    ap.add_argument("--max-depth", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scenes", default="final_scene1,suzanne")
    ap.add_argument("--target-spp", type=int, default=64)
    ap.add_argument("--max-samples", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import raytracinginaweekend_amd as R

    size = R.Size2i(a.width, a.height)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        r = fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1), r

    def med(v):
        return sorted(v)[len(v) // 2]

    def spread(v):
        return (max(v) - min(v)) / med(v)

    # ---- 1. overhead while nothing stops --------------------------------------------------------------
    world = R.demo_world("final_scene1")
    dws = {"plain": R.DeviceWorld(world, 0), "adaptive": R.DeviceWorld(world, 0)}

    def adds(name):
        acc = R.Accumulator(dws[name], size, a.max_depth, moments=True, adaptive=name == "adaptive")

        def run():
            while acc.samples < a.spp:
                acc.add(min(a.add, a.spp - acc.samples), sp)
                if name == "adaptive":
                    assert acc.adapt(0.0, 2, sp)[0] == acc.tiles, "target 0 must stop nothing"

        ms, _ = timed(run)
        lf = dws[name].last_frame()
        assert acc.samples == a.spp
        alone = None
        if name == "adaptive":  # the adapt call alone, on an idle device
            host, dev = [], []
            for _ in range(9):
                torch.cuda.synchronize()
                h0 = time.perf_counter()
                dev.append(timed(lambda: acc.adapt(0.0, 2, sp))[0])
                host.append((time.perf_counter() - h0) * 1e3)
            alone = (med(host), med(dev))
        acc.release()
        return ms, alone, lf["launches"]

    for name in dws:
        adds(name)
    ms = {n: [] for n in dws}
    launches = {}
    for _ in range(a.rounds):
        for name in dws:
            t, alone, launches[name] = adds(name)
            ms[name].append(t)
            if alone:
                adapt_alone = alone
    n_adds = -(-a.spp // a.add)
    say(f"1. overhead while nothing stops: final_scene1 {a.width}x{a.height}, {n_adds} adds of {a.add} to {a.spp} spp, max_depth "
        f"{a.max_depth}, {a.rounds} alternating rounds, ms (device events), one resident world per variant")
    say(f"plain moments accumulator (yardstick): {' '.join(f'{t:.2f}' for t in ms['plain'])}  median {med(ms['plain']):.2f}  "
        f"[last add: launches {launches['plain']}]")
    say(f"adaptive, adapt(target 0) per add:     {' '.join(f'{t:.2f}' for t in ms['adaptive'])}  median {med(ms['adaptive']):.2f}  "
        f"[last add: launches {launches['adaptive']}]")
    say(f"adaptive / plain {med(ms['adaptive']) / med(ms['plain']):.4f}   spread of plain (max - min) / median {spread(ms['plain']):.4f}   "
        f"per add {(med(ms['adaptive']) - med(ms['plain'])) / n_adds:.3f} ms")
    say(f"one adapt call alone on an idle device (median of 9): {adapt_alone[0]:.3f} ms host clock (two event records, test kernel, "
        f"copy of the stop map, synchronise, the host's count), {adapt_alone[1]:.3f} ms between device events")
    for d in dws.values():
        d.release()

    # ---- 2. equal-target cost ---------------------------------------------------------------------------
    say("")
    say(f"2. equal-target cost at {a.width}x{a.height}, max_depth {a.max_depth}: target = noise() of a uniform {a.target_spp} spp frame, "
        f"batch {a.batch}, at most {a.max_samples} spp, {a.rounds} alternating rounds, ms (device events)")
    for scene in [s for s in a.scenes.split(",") if s]:
        world = R.demo_world(scene)
        dws = {"uniform": R.DeviceWorld(world, 0), "adaptive": R.DeviceWorld(world, 0)}
        acc = R.Accumulator(dws["uniform"], size, a.max_depth, moments=True)
        acc.add(a.target_spp)
        target = acc.noise()[0]
        acc.release()

        def uniform():
            img, n, noise = R.render_to_noise(size, a.max_depth, dws["uniform"], target, a.max_samples, batch=a.batch)
            return {"samples": n, "samples_rendered": n * size.count(), "active_tiles": None, "noise": noise}

        def adaptive():
            img, counts, info = R.render_adaptive(size, a.max_depth, dws["adaptive"], target, a.max_samples,
                                                  min_samples=a.batch, batch=a.batch)
            info["histogram"] = dict(zip(*[x.tolist() for x in np.unique(counts, return_counts=True)]))
            return info

        reached = adaptive()["noise"]  # (also the adaptive variant's warm-up)

        def uniform_eq():
            img, n, noise = R.render_to_noise(size, a.max_depth, dws["uniform"], reached, 2 * a.max_samples, batch=a.batch)
            return {"samples": n, "samples_rendered": n * size.count(), "active_tiles": None, "noise": noise}

        fns = {"uniform": uniform, "adaptive": adaptive, "uniform to the adaptive frame's noise()": uniform_eq}
        uniform()
        uniform_eq()
        ms, res = {n: [] for n in fns}, {}
        for _ in range(a.rounds):
            for name, fn in fns.items():
                t, res[name] = timed(fn)
                ms[name].append(t)
        say(f"{scene}: target {target:.6f}")
        for name in fns:
            r = res[name]
            say(f"  {name}: {' '.join(f'{t:.2f}' for t in ms[name])}  median {med(ms[name]):.2f} ms  frontier {r['samples']} spp  "
                f"samples rendered {r['samples_rendered']} ({r['samples_rendered'] / size.count():.2f} per pixel)  noise() {r['noise']:.6f}"
                + (f"  active tiles at the end {r['active_tiles']}" if r["active_tiles"] is not None else ""))
        say(f"  pixels per sample count (adaptive): {res['adaptive']['histogram']}")
        say(f"  adaptive / uniform: time {med(ms['adaptive']) / med(ms['uniform']):.4f}  samples "
            f"{res['adaptive']['samples_rendered'] / res['uniform']['samples_rendered']:.4f}   spread of uniform {spread(ms['uniform']):.4f}")
        eq = "uniform to the adaptive frame's noise()"
        say(f"  adaptive / {eq}: time {med(ms['adaptive']) / med(ms[eq]):.4f}  samples "
            f"{res['adaptive']['samples_rendered'] / res[eq]['samples_rendered']:.4f}   spread of the latter {spread(ms[eq]):.4f}")
        for d in dws.values():
            d.release()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
