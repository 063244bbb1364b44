"""What a denoised preview costs and what it buys, on one GPU in one process.

(a) Time.  Device events around one `Denoiser.run_device` at `--width` x `--height` for iterations 1..5, guided
    (3 channels) and unguided, on a 16-spp final_scene1 frame: `--warmup` runs, then the median of `--runs` with the
    spread (max - min) / median, beside the compulsory-bytes bound (prep: inputs read, records and guide written;
    per level 32 B read + 16 B written per pixel, 16 + 16 unguided; the last level writes 12 or 16 B) at
    `--hbm-gbs`, and beside the time of a 16-spp add on the same world.
(b) Quality.  At the same size, 8 and 32 spp (seed 31) of `--scenes`: MSE (squared error summed over the channels,
    averaged over the pixels) and rel (the squared error divided by the reference pixel's squared norm + 0.01,
    averaged) of the noisy frame and of the denoised one, with the Normals guide and without, against a
    `--ref-spp` frame of seed 977 rendered by the product.  Pixels whose error is not finite are left out of both
    means and counted.  No thresholds: a table.

python tools/denoise_bench.py [--out profiles/r10/denoise_bench.txt]
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the bound is computed at")
    ap.add_argument("--scenes", default="final_scene1,cornell_box,earth_mapped,suzanne")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import raytracinginaweekend_amd as R

    size = R.Size2i(a.width, a.height)
    n = size.count()
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    lines = []

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

    def frame(dworld, spp, seed, mode=R.RenderMode.Default, moments=False):
        """(image, stderr or None) of a frame as device tensors."""
        acc = R.Accumulator(dworld, size, a.max_depth, mode, seed=seed, moments=moments)
        acc.add(spp, sp)
        image = acc._resolved_device(R._native.lib().rtw_accum_resolve)
        se = acc._resolved_device(R._native.lib().rtw_accum_resolve_stderr) if moments else None
        torch.cuda.synchronize()
        acc.release()
        return image, se

    den = R.Denoiser(size)

    # ---- (a) time -----------------------------------------------------------------------------------------
    dworld = R.DeviceWorld(R.demo_world("final_scene1"), 0)
    color, se = frame(dworld, 16, 31, moments=True)
    normals, _ = frame(dworld, 16, 31, R.RenderMode.Normals)
    out = torch.empty_like(color)
    say(f"(a) time of one Denoiser run at {a.width}x{a.height} on a 16-spp final_scene1 frame: device events, {a.warmup} warm-up "
        f"runs, median of {a.runs}, spread = (max - min) / median; bound = compulsory bytes at {a.hbm_gbs:.0f} GB/s")
    say("guide      iterations  median ms  min ms   max ms   spread  compulsory MB  bound ms  median / bound")
    for guided in (True, False):
        for it in range(1, 6):
            g = normals if guided else None
            run = lambda: den.run_device(color, se, g, out, iterations=it, stream_ptr=sp)  # noqa: E731
            for _ in range(a.warmup):
                run()
            torch.cuda.synchronize()
            ms = [timed(run) for _ in range(a.runs)]
            gb = 12 if guided else 0
            # prep: colour, error and guide in, record (and padded guide) out; levels: records (and guides) in,
            # records out, the last one the 12-byte image
            bytes_ = n * ((24 + gb + 16 + (16 if guided else 0)) + it * (32 if guided else 16) + (it - 1) * 16 + 12)
            bound = bytes_ / (a.hbm_gbs * 1e9) * 1e3
            say(f"{'normals' if guided else 'none':<10} {it:<11d} {med(ms):<10.4f} {min(ms):<8.4f} {max(ms):<8.4f} "
                f"{(max(ms) - min(ms)) / med(ms):<7.3f} {bytes_ / 1e6:<14.1f} {bound:<9.4f} {med(ms) / bound:.2f}")
    acc = R.Accumulator(dworld, size, a.max_depth, seed=31, moments=True)
    acc.add(16, sp)  # (warm-up: the world learns its tile order)
    torch.cuda.synchronize()
    adds = [timed(lambda: acc.add(16, sp)) for _ in range(5)]
    say(f"a 16-spp add (moments) on the same world and size: median {med(adds):.2f} ms of 5 ({' '.join(f'{t:.2f}' for t in adds)})")
    acc.release()
    dworld.release()

    # ---- (b) quality --------------------------------------------------------------------------------------
    if not a.skip_quality:
        say("")
        say(f"(b) quality at {a.width}x{a.height}, max_depth {a.max_depth}: frames of seed 31 against a {a.ref_spp}-spp frame of seed "
            f"977 (both rendered by the product); defaults (iterations 3, sigma_l 1.5, sigma_g 0.35); MSE = squared error summed "
            f"over the channels, averaged over the pixels; rel = squared error / (|reference|^2 + 0.01), averaged")
        say("world          spp  metric  noisy        denoised+normals  denoised unguided  pixels left out of the means")
        for scene in [s for s in a.scenes.split(",") if s]:
            dworld = R.DeviceWorld(R.demo_world(scene), 0)
            ref = frame(dworld, a.ref_spp, 977)[0].double()
            ref_norm = (ref * ref).sum(dim=1) + 0.01
            for spp in (8, 32):
                color, se = frame(dworld, spp, 31, moments=True)
                normals, _ = frame(dworld, spp, 31, R.RenderMode.Normals)
                imgs = {"noisy": color, "guided": den.run_device(color, se, normals), "plain": den.run_device(color, se)}
                torch.cuda.synchronize()
                err = {k: ((v.double() - ref) ** 2).sum(dim=1) for k, v in imgs.items()}
                ok = torch.isfinite(err["noisy"]) & torch.isfinite(err["guided"]) & torch.isfinite(err["plain"])
                bad = int((~ok).sum())
                mse = {k: float(e[ok].mean()) for k, e in err.items()}
                rel = {k: float((e / ref_norm)[ok].mean()) for k, e in err.items()}
                for metric, v in (("MSE", mse), ("rel", rel)):
                    say(f"{scene:<14} {spp:<4d} {metric:<7} {v['noisy']:<12.6f} {v['guided']:<17.6f} {v['plain']:<18.6f} {bad}")
            dworld.release()
    den.release()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
