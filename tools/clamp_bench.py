"""What sample clamping (RTW_ACCUM_CLAMP) costs and what it buys, on one GPU.

(a) cost: 8 adds of 64 samples at 1920x1080, a clamp+finite+moments accumulator against a finite+moments
    accumulator, device events around the adds, three alternating rounds in one process after a warm-up of each,
    each variant on its own resident world (the set-up of tools/finite_bench.py); final_scene1 with L = 0.5 (heavy
    clamping), then cornell_box with L = 1.0.  With --parent-library the yardstick is the parent commit's library
    (tools/build_head_variant.sh): three more rounds alternate a fresh process on that library (finite only) with a
    fresh process on this one, which also shows what a finite accumulator's add costs here against the parent.
    The clamp pass moves 32 B more state per slot and launch (clamped 8 B, lost 24 B) beside 768 B of colours.
(b) what it buys: render_adaptive on cornell_box at 640x360, target 0.05, with and without clamp = 4.0: the samples
    spent, the tiles still active at the cap, and the mean of clamp_loss() against the mean image.  Reported as found.

python tools/clamp_bench.py [--parent-library raytracinginaweekend_amd/librtw_head.so] [--out profiles/r20/clamp_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, DEPTH, ADDS, PER_ADD = 1920, 1080, 50, 8, 64
SCENES = (("final_scene1", 0.5), ("cornell_box", 1.0))


def timed_adds(R, torch, dw, size, variant, level, adds=ADDS):
    """ms of `adds` adds of 64 samples on a fresh accumulator (its buffers are made outside the timed span)."""
    acc = R.Accumulator(dw, size, DEPTH, moments=True, **({"clamp": level} if variant == "clamp" else {"finite": True}))
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(adds):
        acc.add(PER_ADD, stream.cuda_stream)
    t1.record(stream)
    t1.synchronize()
    acc.release()
    return t0.elapsed_time(t1)


def child_cost(a):
    """One process: warm-up of each variant, then `rounds` alternating rounds; one JSON line."""
    import torch

    import raytracinginaweekend_amd as R

    size, world = R.Size2i(a.width, a.height), R.demo_world(a.scene)
    variants = a.variants.split(",")
    dws = {v: R.DeviceWorld(world, 0) for v in variants}
    for v in variants:  # buffers grown, threshold tuned, tile order learned
        for _ in range(a.warmup):
            timed_adds(R, torch, dws[v], size, v, a.level, a.adds)
    ms = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            ms[v].append(timed_adds(R, torch, dws[v], size, v, a.level, a.adds))
    print(json.dumps(ms), flush=True)


def child_benefit(a):
    import numpy as np
    import torch  # noqa: F401  (first: librtw.so then binds the HIP runtime torch ships)

    import raytracinginaweekend_amd as R

    size, dw = R.Size2i(640, 360), R.DeviceWorld(R.demo_world("cornell_box"), 0)
    rows = []
    for clamp in (None, 4.0):
        acc = R.Accumulator(dw, size, DEPTH, seed=7, adaptive=True, finite=True, **({"clamp": clamp} if clamp else {}))
        active = acc.tiles
        while active > 0 and acc.samples < a.max_samples:  # render_adaptive's loop, the accumulator kept for the loss
            acc.add(min(16, a.max_samples - acc.samples))
            active = acc.adapt(0.05, 16)[0]
        image = acc.image()
        row = {"clamp": clamp, "samples_spent": int(acc.sample_counts().astype(np.int64).sum()), "frontier": acc.samples,
               "active_tiles": active, "tiles": acc.tiles, "noise": acc.noise()[0], "mean_image": float(image.astype(np.float64).mean())}
        if clamp:
            row["mean_loss"] = float(acc.clamp_loss().astype(np.float64).mean())
            row["clamped_samples"] = int(acc.clamped_counts().astype(np.int64).sum())
        rows.append(row)
        acc.release()
    print(json.dumps(rows), flush=True)


def run_child(args, library=None):
    env = dict(os.environ)
    env.pop("RTW_LIBRARY", None)
    if library:
        env["RTW_LIBRARY"] = os.path.abspath(library)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), *args], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=400)
    if out.returncode != 0:  # (ends the whole run: nothing more is started on the GPU after a child that failed)
        sys.exit(f"clamp_bench: child {args} ended with status {out.returncode}\n{out.stderr[-3000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith(("{", "["))][-1])


def spread(v):
    return (max(v) - min(v)) / sorted(v)[len(v) // 2]


def med(v):
    return sorted(v)[len(v) // 2]


def fmt(v):
    return " ".join(f"{t:.2f}" for t in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--scene", default="final_scene1")
    ap.add_argument("--level", type=float, default=0.5)
    ap.add_argument("--variants", default="finite,clamp")
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--adds", type=int, default=ADDS)
    ap.add_argument("--max-samples", type=int, default=1024)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--no-benefit", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child == "cost":
        return child_cost(a)
    if a.child == "benefit":
        return child_benefit(a)
    lines = [f"sample clamping, {a.width}x{a.height}, max_depth {DEPTH}, ms (device events) of {a.adds} adds of {PER_ADD} samples;",
             "finite = a finite+moments accumulator, clamp = clamp+finite+moments; one resident world per variant"]
    geom = ["--width", str(a.width), "--height", str(a.height), "--adds", str(a.adds)]

    def write():
        text = "\n".join(lines)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return text

    for scene, level in SCENES:
        lines.append(f"## (a) {scene}, L = {level}")
        where = ["--scene", scene, "--level", str(level), *geom]
        ms = run_child(["--child", "cost", *where])
        lines += [f"one process, 3 alternating rounds   finite {fmt(ms['finite'])}  median {med(ms['finite']):.2f}",
                  f"                                    clamp  {fmt(ms['clamp'])}  median {med(ms['clamp']):.2f}",
                  f"clamp / finite {med(ms['clamp']) / med(ms['finite']):.4f}   spread of finite (max - min) / median {spread(ms['finite']):.4f}"]
        if a.parent_library:
            par, bf, bc = [], [], []
            for _ in range(3):  # a fresh process per library, alternated
                par += run_child(["--child", "cost", "--variants", "finite", "--rounds", "1", *where], a.parent_library)["finite"]
                b = run_child(["--child", "cost", "--rounds", "1", *where])
                bf += b["finite"]
                bc += b["clamp"]
            lines += [f"parent's library, finite            {fmt(par)}  median {med(par):.2f}  spread {spread(par):.4f}",
                      f"this library, finite                {fmt(bf)}  median {med(bf):.2f}  ({med(bf) / med(par):.4f} of the parent)",
                      f"this library, clamp                 {fmt(bc)}  median {med(bc):.2f}",
                      f"COST clamp / parent's finite {med(bc) / med(par):.4f}"]
        write()
    if not a.no_benefit:
        lines.append(f"## (b) render_adaptive's loop on cornell_box, 640x360, seed 7, target 0.05, batch 16, cap {a.max_samples}")
        for r in run_child(["--child", "benefit", "--max-samples", str(a.max_samples)]):
            line = (f"clamp {r['clamp']}: samples spent {r['samples_spent']} (frontier {r['frontier']}), tiles active at the end "
                    f"{r['active_tiles']} of {r['tiles']}, noise {r['noise']:.6f}, mean image {r['mean_image']:.6f}")
            if r["clamp"]:
                line += (f", mean clamp_loss {r['mean_loss']:.6f} = {r['mean_loss'] / r['mean_image']:.4f} of the mean image, "
                         f"{r['clamped_samples']} clamped samples")
            lines.append(line)
    print(write(), flush=True)


if __name__ == "__main__":
    main()
