"""What the first-hit AOV pass costs and what albedo demodulation buys, on one GPU in one process.

(a) Time.  Device events around one add of n samples at `--width` x `--height`, n = 4 and 64, on `--scenes`:
    `AovAccumulator.add(n)`, `Accumulator(Default).add(n)` and `Accumulator(Normals).add(n)`, all three on one
    resident world.  `--warmup` adds, then the median of `--runs`, in `--rounds` alternating rounds (AOV, Default,
    Normals, AOV, ...) in one run; the table holds each round's median and the median of those.  Every add renders
    new samples (the accumulators grow), as a progressive frame does.
    Gate: the AOV add must be faster than the Default add of the same n on final_scene1 and on earth_mapped -- it
    traces a strict subset of that add's rays.  The ratio to the Normals add (the megakernel, the SAH tree in LDS)
    is recorded only.  The exit status is 1 when the gate fails; the table is written either way.
(b) Quality.  tools/denoise_bench.py's table with a third column: at the same size, 8 and 32 spp (seed 31) of each
    scene against a `--ref-spp` frame of seed 977 rendered by the product, the noisy frame, today's filter (Normals
    guide of the frame's spp) and the demodulated filter (the same guide, the albedo of a `--aov-spp` AOV
    accumulator of seed 31).  MSE = squared error summed over the channels, averaged over the pixels; rel = squared
    error / (|reference|^2 + 0.01), averaged.  Pixels whose error is not finite in any column are left out of all
    and counted.  No thresholds: a table.

python tools/aov_bench.py [--out profiles/r11/aov_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--max-depth", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scenes", default="final_scene1,earth_mapped,cornell_box,suzanne")
    ap.add_argument("--gated", default="final_scene1,earth_mapped")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--aov-spp", type=int, default=64)
    ap.add_argument("--skip-time", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import raytracinginaweekend_amd as R

    size = R.Size2i(a.width, a.height)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    lines = []
    failed = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    def med(v):
        return sorted(v)[len(v) // 2]

    scenes = [s for s in a.scenes.split(",") if s]
    lib = R._native.lib()

    # ---- (a) time -----------------------------------------------------------------------------------------
    if not a.skip_time:
        say(f"(a) one add of n samples at {a.width}x{a.height}, max_depth {a.max_depth}, seed 31: device events, {a.warmup} warm-up "
            f"adds, median of {a.runs}, {a.rounds} alternating rounds in one run; ms")
        say("world          n    add       " + "  ".join(f"round {r + 1:<3d}" for r in range(a.rounds)) + "  median    AOV / this")
        for scene in scenes:
            dworld = R.DeviceWorld(R.demo_world(scene), 0)
            for n in (4, 64):
                adders = {
                    "AOV": R.AovAccumulator(dworld, size, seed=31),
                    "Default": R.Accumulator(dworld, size, a.max_depth, seed=31),
                    "Normals": R.Accumulator(dworld, size, a.max_depth, R.RenderMode.Normals, seed=31),
                }
                rounds = {k: [] for k in adders}
                for _ in range(a.rounds):
                    for k, acc in adders.items():
                        for _ in range(a.warmup):
                            acc.add(n, sp)
                        torch.cuda.synchronize()
                        rounds[k].append(med([timed(lambda: acc.add(n, sp)) for _ in range(a.runs)]))
                m = {k: med(v) for k, v in rounds.items()}
                for k in adders:
                    say(f"{scene:<14} {n:<4d} {k:<9} " + "  ".join(f"{t:<9.4f}" for t in rounds[k]) +
                        f"  {m[k]:<9.4f} {m['AOV'] / m[k]:.3f}")
                if scene in a.gated.split(","):
                    ok = m["AOV"] < m["Default"]
                    say(f"{scene:<14} {n:<4d} gate: AOV add faster than the Default add: {'yes' if ok else 'NO'}")
                    if not ok:
                        failed.append((scene, n))
                for acc in adders.values():
                    acc.release()
            dworld.release()

    # ---- (b) quality --------------------------------------------------------------------------------------
    if not a.skip_quality:
        def frame(dworld, spp, seed, mode=R.RenderMode.Default, moments=False):
            acc = R.Accumulator(dworld, size, a.max_depth, mode, seed=seed, moments=moments)
            acc.add(spp, sp)
            image = acc._resolved_device(lib.rtw_accum_resolve)
            se = acc._resolved_device(lib.rtw_accum_resolve_stderr) if moments else None
            torch.cuda.synchronize()
            acc.release()
            return image, se

        den = R.Denoiser(size)
        say("")
        say(f"(b) quality at {a.width}x{a.height}, max_depth {a.max_depth}: frames of seed 31 against a {a.ref_spp}-spp frame of seed "
            f"977 (both rendered by the product); defaults (iterations 3, sigma_l 1.5, sigma_g 0.35), Normals guide of the "
            f"frame's spp; demodulated: the albedo of a {a.aov_spp}-spp AOV accumulator of seed 31; MSE = squared error summed "
            f"over the channels, averaged over the pixels; rel = squared error / (|reference|^2 + 0.01), averaged")
        say("world          spp  metric  noisy        today's filter  demodulated   demodulated / noisy  / today's  pixels left out")
        for scene in scenes:
            dworld = R.DeviceWorld(R.demo_world(scene), 0)
            ref = frame(dworld, a.ref_spp, 977)[0].double()
            ref_norm = (ref * ref).sum(dim=1) + 0.01
            aov = R.AovAccumulator(dworld, size, seed=31, channels=("albedo",))
            aov.add(a.aov_spp, sp)
            albedo = aov.albedo_device()
            for spp in (8, 32):
                color, se = frame(dworld, spp, 31, moments=True)
                normals, _ = frame(dworld, spp, 31, R.RenderMode.Normals)
                imgs = {"noisy": color, "today": den.run_device(color, se, normals),
                        "demod": den.run_device(color, se, normals, albedo=albedo)}
                torch.cuda.synchronize()
                err = {k: ((v.double() - ref) ** 2).sum(dim=1) for k, v in imgs.items()}
                ok = torch.isfinite(err["noisy"]) & torch.isfinite(err["today"]) & torch.isfinite(err["demod"])
                bad = int((~ok).sum())
                mse = {k: float(e[ok].mean()) for k, e in err.items()}
                rel = {k: float((e / ref_norm)[ok].mean()) for k, e in err.items()}
                for metric, v in (("MSE", mse), ("rel", rel)):
                    say(f"{scene:<14} {spp:<4d} {metric:<7} {v['noisy']:<12.6f} {v['today']:<15.6f} {v['demod']:<13.6f} "
                        f"{v['demod'] / v['noisy']:<20.3f} {v['demod'] / v['today']:<10.3f} {bad}")
            aov.release()
            dworld.release()
        den.release()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if failed:
        print(f"gate failed: {failed}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
