"""What bringing partition accumulators together costs, on one GPU in one process.

Eight partition accumulators (moments + finite) of one resident world at 1920x1080 are each packed into one
gathered buffer (rtw_accum_pack x 8) and the buffer is merged into the whole image's accumulator
(rtw_accum_merge_parts, one launch; the span includes its read-back of the eight headers).  Beside them, in the
same run: `whole.add(16)` and one rtw_accum_resolve of the same frame.  Alternated `--rounds` times after a
warm-up of each, timed with device events around work that ends in a synchronise.  The 16-byte path and, forced
with RTW_PARTS_DWORD=1, the dword path are both timed.

The gather itself (RCCL over xGMI between GPUs) cannot be timed on one GPU: here the records are packed straight
into the gathered buffer.

python tools/parts_bench.py [--out profiles/r13/parts_bench.txt]
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
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--add", type=int, default=16)
    ap.add_argument("--max-depth", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import raytracinginaweekend_amd as R
    from raytracinginaweekend_amd import _native as N

    size = R.Size2i(a.width, a.height)
    dw = R.DeviceWorld(R.demo_world(a.scene), 0)
    kw = dict(moments=True, finite=True)
    parts = [R.Accumulator(dw, size, a.max_depth, part=(r, a.parts), layout=N.LAYOUT_TILES, **kw) for r in range(a.parts)]
    whole = R.Accumulator(dw, size, a.max_depth, **kw)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    for p in parts:
        p.add(1, sp)
    stride = -(-parts[0].packed_bytes() // 16) * 16
    words = stride // 4
    gathered = torch.zeros(a.parts * words, dtype=torch.int32, device="cuda:0")
    out = torch.zeros(size.count() * 3, dtype=torch.float32, device="cuda:0")
    state_bytes = whole.slots * (12 + 12 + 4)

    def pack():
        for r, p in enumerate(parts):
            p.pack_into(gathered[r * words: (r + 1) * words], sp)

    def merge():
        whole.merge_parts(gathered, stride, a.parts, sp)

    def add():
        whole.add(a.add, sp)

    def resolve():
        whole.resolve_into(out.data_ptr(), sp)

    def timed(fn):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    def dword(fn):
        def run():
            os.environ["RTW_PARTS_DWORD"] = "1"
            try:
                fn()
            finally:
                del os.environ["RTW_PARTS_DWORD"]
        return run

    variants = [("pack", pack), ("merge", merge), ("pack_dword", dword(pack)), ("merge_dword", dword(merge)), ("add", add),
                ("resolve", resolve)]
    for _, fn in variants:  # warm-up (the add's too: buffers grown, threshold tuned, tile order learned)
        for _ in range(2):
            timed(fn)
    ms = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            ms[name].append(timed(fn))
    med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}

    def row(label, name, traffic=None):
        rate = f"  {2 * traffic / med[name] / 1e6:.0f} GB/s read + written" if traffic else ""
        return f"{label:<34}{' '.join(f'{t:.3f}' for t in ms[name])}  median {med[name]:.3f}{rate}"

    resolve_bytes = whole.slots * (12 + 4) + size.count() * 12  # sums and kept read, the image written
    lines = [f"{a.scene} {a.width}x{a.height} max_depth {a.max_depth}, flags moments+finite, {a.parts} parts of one resident world, "
             f"{a.rounds} alternating rounds, ms (device events)",
             f"state {state_bytes / 1e6:.1f} MB, record {parts[0].packed_bytes()} B at a stride of {stride} B",
             row(f"pack x {a.parts} (16-byte path):", "pack", state_bytes),
             row("merge, 1 launch (16-byte path):", "merge", state_bytes),
             row(f"pack x {a.parts} (dword path, forced):", "pack_dword", state_bytes),
             row("merge, 1 launch (dword, forced):", "merge_dword", state_bytes),
             row(f"whole.add({a.add}):", "add"),
             row("whole resolve:", "resolve"),
             f"(pack + merge) / add({a.add}) {(med['pack'] + med['merge']) / med['add']:.5f}   "
             f"(pack + merge) / resolve {(med['pack'] + med['merge']) / med['resolve']:.2f}   "
             f"bytes moved, (pack + merge) / resolve {4 * state_bytes / resolve_bytes:.2f}",
             "not measured: the gather between GPUs (RCCL over xGMI); one GPU holds all parts here"]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
