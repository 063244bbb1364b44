"""What finite-sample accumulation (RTW_ACCUM_FINITE) costs and what it buys, on one GPU.

(a) cost: 8 adds of 64 samples at 1920x1080, a finite+moments accumulator against a plain moments accumulator,
    device events around the adds, three alternating rounds in one process after a warm-up of each, each variant
    on its own resident world (the set-up of tools/accum_bench.py); final_scene1, then suzanne.  With
    --parent-library the yardstick is the parent commit's library (tools/build_head_variant.sh): three more
    rounds alternate a fresh process on that library (plain moments only) with a fresh process on this one.
    One `rocprofv3 --kernel-trace` run of eight adds per variant gives the accumulate pass's own time and from
    it the bandwidth of the pass and what the kept array's 8 B per slot and launch amount to.
(b) what it buys: suzanne 1920x1080 at 64 and 512 spp, plain moments against finite+moments: pixels with a
    non-finite channel in the plain image, pixels with kept == 0, rejected samples, noise() and its pixel count.

python tools/finite_bench.py [--parent-library raytracinginaweekend_amd/librtw_head.so] [--out profiles/r12/finite_bench.txt]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, DEPTH, ADDS, PER_ADD = 1920, 1080, 50, 8, 64


def timed_adds(R, torch, dw, size, variant, adds=ADDS):
    """ms of `adds` adds of 64 samples on a fresh accumulator (its buffers are made outside the timed span)."""
    acc = R.Accumulator(dw, size, DEPTH, moments=True, **({"finite": True} if variant == "finite" else {}))
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
            timed_adds(R, torch, dws[v], size, v, a.adds)
    ms = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            ms[v].append(timed_adds(R, torch, dws[v], size, v, a.adds))
    print(json.dumps(ms), flush=True)


def child_quality(a):
    import numpy as np
    import torch  # noqa: F401  (first: librtw.so then binds the HIP runtime torch ships)

    import raytracinginaweekend_amd as R

    size, world = R.Size2i(a.width, a.height), R.demo_world("suzanne")
    dw = R.DeviceWorld(world, 0)
    plain = R.Accumulator(dw, size, DEPTH, seed=7, moments=True)
    fin = R.Accumulator(dw, size, DEPTH, seed=7, moments=True, finite=True)
    rows, done = [], 0
    for spp in (64, 512):
        plain.add(spp - done)
        fin.add(spp - done)
        done = spp
        holes = int((~np.isfinite(plain.image())).any(axis=1).sum())
        kept = fin.kept_counts()
        pn, fn = plain.noise(), fin.noise()
        rows.append({"spp": spp, "pixels": size.count(), "plain_nonfinite_pixels": holes,
                     "finite_nonfinite_pixels": int((~np.isfinite(fin.image())).any(axis=1).sum()),
                     "kept0_pixels": int((kept == 0).sum()), "rejected_samples": int(fin.rejected_counts().astype(np.int64).sum()),
                     "plain_noise": pn[0], "plain_pixels_counted": pn[1], "finite_noise": fn[0], "finite_pixels_counted": fn[1]})
    print(json.dumps(rows), flush=True)


def run_child(args, library=None, prefix=()):
    env = dict(os.environ)
    env.pop("RTW_LIBRARY", None)
    if library:
        env["RTW_LIBRARY"] = os.path.abspath(library)
    out = subprocess.run([*prefix, sys.executable, os.path.abspath(__file__), *args], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    if out.returncode != 0:  # (ends the whole run: nothing more is started on the GPU after a child that failed)
        sys.exit(f"finite_bench: child {args} ended with status {out.returncode}\n{out.stderr[-3000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith(("{", "["))][-1])


def spread(v):
    return (max(v) - min(v)) / sorted(v)[len(v) // 2]


def med(v):
    return sorted(v)[len(v) // 2]


def fmt(v):
    return " ".join(f"{t:.2f}" for t in v)


def pass_times(scene, geom):
    """Per-launch time (us) of the two accumulate kernels, from one rocprofv3 --kernel-trace run; None if the
    profiler is absent or its output holds no row of them."""
    if not shutil.which("rocprofv3"):
        return None
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        # (a child that fails ends the whole run: nothing more is started on the GPU after it)
        run_child(["--child", "cost", "--scene", scene, "--variants", "plain,finite", "--warmup", "0", "--rounds", "1", *geom],
                  prefix=("rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "kt", "--"))
        times = {"accumulate_moments_kernel": [], "accumulate_finite_kernel": []}
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for k in times:
                    if k in row.get("Kernel_Name", ""):
                        times[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return times if all(times.values()) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--scene", default="final_scene1")
    ap.add_argument("--variants", default="plain,finite")
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--adds", type=int, default=ADDS)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child == "cost":
        return child_cost(a)
    if a.child == "quality":
        return child_quality(a)
    slots = a.width * a.height  # (1920x1080 in 8x8 tiles: no padding slot)
    lines = [f"finite-sample accumulation, {a.width}x{a.height}, max_depth {DEPTH}, ms (device events) of {ADDS} adds of {PER_ADD} samples;",
             "plain = a moments accumulator, finite = finite+moments; one resident world per variant"]
    geom = ["--width", str(a.width), "--height", str(a.height)]
    results = {}

    def write():
        text = "\n".join(lines)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return text

    for scene in ("final_scene1", "suzanne"):
        lines.append(f"## (a) {scene}")
        ms = run_child(["--child", "cost", "--scene", scene, *geom])
        lines += [f"one process, 3 alternating rounds   plain  {fmt(ms['plain'])}  median {med(ms['plain']):.2f}",
                  f"                                    finite {fmt(ms['finite'])}  median {med(ms['finite']):.2f}",
                  f"finite / plain {med(ms['finite']) / med(ms['plain']):.4f}   spread of plain (max - min) / median {spread(ms['plain']):.4f}"]
        if a.parent_library:
            par, bp, bf = [], [], []
            for _ in range(3):  # a fresh process per library, alternated
                par += run_child(["--child", "cost", "--scene", scene, "--variants", "plain", "--rounds", "1", *geom], a.parent_library)["plain"]
                b = run_child(["--child", "cost", "--scene", scene, "--rounds", "1", *geom])
                bp += b["plain"]
                bf += b["finite"]
            lines += [f"parent's library, plain             {fmt(par)}  median {med(par):.2f}  spread {spread(par):.4f}",
                      f"this library, plain                 {fmt(bp)}  median {med(bp):.2f}  ({med(bp) / med(par):.4f} of the parent)",
                      f"this library, finite                {fmt(bf)}  median {med(bf):.2f}",
                      f"COST finite / parent's plain {med(bf) / med(par):.4f}"]
        results[scene] = (par, bf) if a.parent_library else None
    write()
    if not a.no_quality:
        lines.append("## (b) suzanne, seed 7: what it buys")
        for r in run_child(["--child", "quality", *geom]):
            lines.append(f"{r['spp']:4d} spp: plain image {r['plain_nonfinite_pixels']} of {r['pixels']} pixels with a non-finite channel "
                         f"(finite image: {r['finite_nonfinite_pixels']}); kept == 0 in {r['kept0_pixels']} pixels; "
                         f"{r['rejected_samples']} rejected samples; noise plain {r['plain_noise']:.6f} over {r['plain_pixels_counted']} pixels, "
                         f"finite {r['finite_noise']:.6f} over {r['finite_pixels_counted']} pixels")

    write()  # (the profiler passes come last: what was measured so far is on disk before them)
    for scene in () if a.no_trace else ("final_scene1", "suzanne"):
        lines.append(f"## (a) {scene}: the accumulate pass alone")
        t = pass_times(scene, geom)
        if t is None:
            lines.append("no kernel trace (rocprofv3 absent, or no row of the accumulate kernels)")
            continue
        pm, fm = med(t["accumulate_moments_kernel"]), med(t["accumulate_finite_kernel"])
        plain_bytes = slots * (12 * PER_ADD + 48)  # colours read; sums and squares read and written
        bw = plain_bytes / (pm * 1e-6) / 1e9
        extra_ms = ADDS * slots * 8 / (bw * 1e9) * 1e3
        lines += [f"per launch (kernel trace, us): accumulate_moments_kernel {fmt(t['accumulate_moments_kernel'])}   "
                  f"accumulate_finite_kernel {fmt(t['accumulate_finite_kernel'])}",
                  f"bandwidth of the plain pass: {plain_bytes / 1e6:.1f} MB / {pm:.1f} us = {bw:.0f} GB/s; kept adds 8 B x {slots} slots "
                  f"x {ADDS} launches = {extra_ms:.4f} ms at that rate; the finite pass takes {fm - pm:+.1f} us per launch "
                  f"({ADDS * (fm - pm) / 1e3:+.4f} ms per {ADDS} adds)"]
        if results.get(scene):
            par, bf = results[scene]
            margin = spread(par) + extra_ms / med(par)
            lines.append(f"MARGIN spread of the parent {spread(par):.4f} + kept traffic {extra_ms / med(par):.5f} = {margin:.4f}; "
                         f"finite / parent's plain - 1 = {med(bf) / med(par) - 1:+.4f}  "
                         f"{'within' if med(bf) / med(par) - 1 <= margin else 'ABOVE'} the margin")
    print(write(), flush=True)


if __name__ == "__main__":
    main()
