"""What partitioning the first-hit AOV pass costs and what a rank's share of it takes, on one GPU.

1920x1080, one add of 64 samples, device events, three alternating rounds; final_scene1 (the leaf-list kernel),
then suzanne (the walk kernel).

(a) the whole-image AOV add on the parent commit's library (--parent-library: a librtw.so built from a checkout of
    the parent, or tools/build_head_variant.sh's) against this tree's: a fresh process per library, alternated, each after one warm-up add.  The change adds
    no work to that path (the partitioned kernel is a template instance of its own), so any excess would be
    register pressure.  GATE: this library's median is at most the parent's median plus the parent's own spread
    (max - min) over its three rounds.
(b) each of the eight parts (r, 8) added alone, against an eighth of this library's whole add.  No gate: a part's
    4 050 waves do not fill one round of the GPU's 5 120 wave slots, and a wave waits for its slowest ray.
(c) pack x 8 and one merge, beside one add and one resolve (albedo), in the same process.

python tools/aov_parts_bench.py --parent-library raytracinginaweekend_amd/librtw_head.so --out profiles/r17/aov_parts_bench.txt
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, N_SAMPLES, PARTS = 1920, 1080, 64, 8


def timed(torch, fn):
    """ms of fn() on the current stream, between device events."""
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1)


def child_whole(a):
    """One process: a warm-up add, then `rounds` whole-image adds, each on a fresh accumulator; one JSON line."""
    import torch

    import raytracinginaweekend_amd as R

    size, dw = R.Size2i(a.width, a.height), R.DeviceWorld(R.demo_world(a.scene), 0)
    ms = []
    for i in range(1 + a.rounds):
        aov = R.AovAccumulator(dw, size, seed=7)
        t = timed(torch, lambda: aov.add(N_SAMPLES))
        aov.release()
        if i > 0:
            ms.append(t)
    print(json.dumps({"whole": ms}), flush=True)


def child_parts(a):
    """One process on this tree's library: whole add, the eight parts' adds, packs, merge and resolve, alternated."""
    import torch

    import raytracinginaweekend_amd as R

    size, dw = R.Size2i(a.width, a.height), R.DeviceWorld(R.demo_world(a.scene), 0)
    out = {"whole": [], "parts": [[] for _ in range(PARTS)], "pack8": [], "merge": [], "resolve": [], "tiles": []}
    for i in range(1 + a.rounds):
        whole = R.AovAccumulator(dw, size, seed=7)
        parts = [R.AovAccumulator(dw, size, seed=7, part=(r, PARTS)) for r in range(PARTS)]
        stride = -(-parts[0].packed_bytes() // 16) * 16
        gathered = torch.zeros(PARTS * stride // 4, dtype=torch.int32, device="cuda:0")
        row = {"whole": timed(torch, lambda: whole.add(N_SAMPLES)),
               "parts": [timed(torch, lambda p=p: p.add(N_SAMPLES)) for p in parts]}
        row["pack8"] = timed(torch, lambda: [p.pack_into(gathered[r * stride // 4: (r + 1) * stride // 4]) for r, p in enumerate(parts)])
        row["merge"] = timed(torch, lambda: whole.merge_parts(gathered, stride, PARTS))
        row["resolve"] = timed(torch, lambda: whole.albedo_device())
        out["tiles"] = [p.tiles for p in parts]
        for acc in parts + [whole]:
            acc.release()
        if i > 0:
            for k in ("whole", "pack8", "merge", "resolve"):
                out[k].append(row[k])
            for r in range(PARTS):
                out["parts"][r].append(row["parts"][r])
    out["record_bytes"] = stride
    print(json.dumps(out), flush=True)


def run_child(args, library=None):
    env = dict(os.environ)
    env.pop("RTW_LIBRARY", None)
    if library:
        env["RTW_LIBRARY"] = os.path.abspath(library)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), *args], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    if out.returncode != 0:  # (ends the whole run: nothing more is started on the GPU after a child that failed)
        sys.exit(f"aov_parts_bench: child {args} ended with status {out.returncode}\n{out.stderr[-3000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def med(v):
    return sorted(v)[len(v) // 2]


def fmt(v):
    return " ".join(f"{t:.2f}" for t in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--scene", default="final_scene1")
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child == "whole":
        return child_whole(a)
    if a.child == "parts":
        return child_parts(a)
    geom = ["--width", str(a.width), "--height", str(a.height)]
    lines = [f"partitioned first-hit AOV pass, {a.width}x{a.height}, ms (device events) of one add of {N_SAMPLES} samples, "
             f"{a.rounds} alternating rounds after one warm-up"]
    ok = True

    def write():
        text = "\n".join(lines)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return text

    for scene in ("final_scene1", "suzanne"):
        lines.append(f"## {scene}")
        if a.parent_library:
            par, own = [], []
            for _ in range(a.rounds):  # a fresh process per library, alternated
                par += run_child(["--child", "whole", "--scene", scene, "--rounds", "1", *geom], a.parent_library)["whole"]
                own += run_child(["--child", "whole", "--scene", scene, "--rounds", "1", *geom])["whole"]
            excess, room = med(own) - med(par), max(par) - min(par)
            within = excess <= room
            ok = ok and within
            lines += [f"(a) whole-image add, parent's library  {fmt(par)}  median {med(par):.2f}  spread (max - min) {room:.2f}",
                      f"(a) whole-image add, this library      {fmt(own)}  median {med(own):.2f}  ({med(own) / med(par):.4f} of the parent)",
                      f"GATE (a) {scene}: this - parent = {excess:+.2f} ms, the parent's spread {room:.2f} ms: "
                      f"{'within' if within else 'ABOVE'}"]
            write()
        p = run_child(["--child", "parts", "--scene", scene, "--rounds", str(a.rounds), *geom])
        eighth = med(p["whole"]) / PARTS
        meds = [med(v) for v in p["parts"]]
        lines += [f"(b) whole-image add, same process      {fmt(p['whole'])}  median {med(p['whole']):.2f}  an eighth {eighth:.2f}",
                  f"(b) tiles of the parts (r, {PARTS})           {' '.join(str(t) for t in p['tiles'])}"]
        lines += [f"(b) part ({r}, {PARTS}) added alone            {fmt(v)}  median {m:.2f}  {m / eighth:.2f} of an eighth"
                  for r, (v, m) in enumerate(zip(p["parts"], meds))]
        lines += [f"(b) a part against an eighth: {min(meds) / eighth:.2f} - {max(meds) / eighth:.2f} "
                  "(the colour accumulators' shares of a frame: 1.07 - 1.11, DESIGN.md 5.5h)",
                  f"(c) pack x {PARTS} {fmt(p['pack8'])}  median {med(p['pack8']):.3f}   merge {fmt(p['merge'])}  median {med(p['merge']):.3f}   "
                  f"resolve (albedo) {fmt(p['resolve'])}  median {med(p['resolve']):.3f}   one add {med(p['whole']):.2f}   "
                  f"record {p['record_bytes']} bytes x {PARTS}"]
        write()
    print(write(), flush=True)
    if not ok:
        sys.exit("aov_parts_bench: gate (a) missed")


if __name__ == "__main__":
    main()
