"""What progressive accumulation costs against the one-shot frame, on one GPU in one process.

Three variants of the same frame (final_scene1 1920x1080x512spp by default), alternated `--rounds` times
after a warm-up of each, timed with device events around work that ends in a synchronise:
  a  the one-shot resident frame (rtw_render_device)
  b  an accumulator: 8 adds of spp / 8 samples, then one resolve
  c  an accumulator: 1 add of spp samples, then one resolve
The yardstick is (a) in the same run; the margin is (a)'s own spread over its rounds.

Each variant renders through its own resident world.  A world keeps one learned tile order
under a key that holds the spp for one-shot frames and 0 for accumulator adds, so one-shot frames and
accumulators that alternate on ONE world each start from chunk-major order again; `--shared-world` measures
that case.

python tools/accum_bench.py [--out profiles/r07/accum_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="final_scene1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--adds", type=int, default=8)
    ap.add_argument("--max-depth", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shared-world", action="store_true", help="all three variants on one resident world")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import raytracinginaweekend_amd as R

    size = R.Size2i(a.width, a.height)
    world = R.demo_world(a.scene)
    shared = R.DeviceWorld(world, 0) if a.shared_world else None
    dws = {name: shared or R.DeviceWorld(world, 0) for name in "abc"}
    out = torch.zeros(size.count() * 3, dtype=torch.float32, device="cuda:0")
    params = R.render_params(size, a.spp, a.max_depth)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    shape = {}

    def one_shot():
        dws["a"].render_into(params, out.data_ptr(), sp)

    def accum(adds):
        def run(acc):
            for i in range(adds):
                acc.add(a.spp * (i + 1) // adds - a.spp * i // adds, sp)
            acc.resolve_into(out.data_ptr(), sp)
        return run

    def timed(name, fn):
        # an accumulator's buffers are allocated (and zeroed) outside the timed span, as the one-shot frame's are
        dw = dws[name]
        acc = R.Accumulator(dw, size, a.max_depth, seed=params.seed) if name != "a" else None
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn(acc) if acc else fn()
        t1.record(stream)
        t1.synchronize()
        lf = dw.last_frame()
        shape[name] = f"launches {lf['launches']}, whole_pixel {lf['whole_pixel']}, trace_min {lf['trace_min']}"
        if acc:
            assert acc.samples == a.spp
            acc.release()
        return t0.elapsed_time(t1)

    variants = [("a", one_shot), ("b", accum(a.adds)), ("c", accum(1))]
    for name, fn in variants:  # warm-up: buffers grown, threshold tuned, tile order learned
        for _ in range(2):
            timed(name, fn)
    ms = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            ms[name].append(timed(name, fn))
    med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
    lines = [f"{a.scene} {a.width}x{a.height}x{a.spp}spp max_depth {a.max_depth}, {a.rounds} alternating rounds, ms (device events), "
             f"{'one resident world for all variants' if a.shared_world else 'one resident world per variant'}",
             f"a one-shot frame:             {' '.join(f'{t:.2f}' for t in ms['a'])}  median {med['a']:.2f}  [{shape['a']}]",
             f"b {a.adds} adds + resolve:          {' '.join(f'{t:.2f}' for t in ms['b'])}  median {med['b']:.2f}  [last add: {shape['b']}]",
             f"c 1 add + resolve:           {' '.join(f'{t:.2f}' for t in ms['c'])}  median {med['c']:.2f}  [{shape['c']}]",
             f"b/a {med['b'] / med['a']:.4f}   c/a {med['c'] / med['a']:.4f}   "
             f"spread of a (max - min) / median {(max(ms['a']) - min(ms['a'])) / med['a']:.4f}"]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
