"""Wall-cycle split of the render kernel's main loop (experiment build only):

  make -C raytracinginaweekend_amd/csrc variant V=pt DEFS=-DRTW_PHASE_TIMING
  RTW_LIBRARY=$PWD/raytracinginaweekend_amd/librtw_pt.so python tools/phase_timing.py --scene final_scene1

Phases (per wave, summed over waves; a wave's cycles include the time other waves on its SIMD
issue; the phase is switched by the wave's first active lane, so divergent sub-phases count whole-wave
cycles): 1 refill (work items), 2 traversal setup (the ray's reciprocals), 3 traversal (SAH walk,
drain, proof, re-traces), 4 shading (hit record, material, texture, pdf), 5 sample start (stream
setup, jitter, camera ray and its UnitDisc), 6 shading's samplers (UnitSphere / UnitBall rejection
loops, gen_bool, light direction), 7 colour store and cost bookkeeping.  The frame after a warm-up
frame (cost order, tuned threshold).
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="final_scene1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=128)
    a = ap.parse_args()
    import torch

    import raytracinginaweekend_amd as R
    from raytracinginaweekend_amd import _native as N

    lib = N.lib()
    fn = lib.rtw_debug_phase_cycles
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong)]
    buf = (C.c_ulonglong * 8)()
    dw = R.DeviceWorld(R.demo_world(a.scene), 0)
    p = R.render_params(R.Size2i(a.width, a.height), a.spp, 50)
    out = torch.empty(a.width * a.height * 3, dtype=torch.float32, device="cuda:0")
    dw.render_into(p, out.data_ptr(), 0)  # warm-up: tuning frame
    torch.cuda.synchronize()
    fx = lib.rtw_debug_phase_extra
    fx.restype = C.c_int
    fx.argtypes = [C.POINTER(C.c_ulonglong)]
    ext = (C.c_ulonglong * 4)()
    fs = lib.rtw_debug_phase_skip
    fs.restype = C.c_int
    fs.argtypes = [C.POINTER(C.c_ulonglong)]
    sk = (C.c_ulonglong * 8)()
    fs(sk)
    fx(ext)
    fn(buf)
    dw.render_into(p, out.data_ptr(), 0)
    torch.cuda.synchronize()
    if fs(sk) != 0 or fx(ext) != 0 or fn(buf) != 0:
        raise SystemExit("library built without RTW_PHASE_TIMING")
    names = {1: "refill", 2: "traversal setup", 3: "traversal", 4: "shading", 5: "sample start",
             6: "samplers", 7: "stores"}
    tot = sum(buf[k] for k in names)
    print(a.scene, f"{a.width}x{a.height}x{a.spp}", " ".join(f"{names[k]} {buf[k] / tot:.4f}" for k in names),
          f"(wave cycles {tot})", flush=True)
    # the leaf-list kernel's camera share of phase 2 (kept apart from the sums above: add it to the total), and
    # the PH_PIXEL lanes a refill round finds (rounds that handed out at least one item)
    tot += ext[0]
    cam, rounds, lanes = ext[0], ext[2], ext[3]
    mean = lanes / rounds if rounds else 0.0
    share = (buf[1] + buf[5] + cam) / tot
    print(f"with the camera set-up: refill {buf[1] / tot:.4f} setup(bounce) {buf[2] / tot:.4f} "
          f"setup(camera) {cam / tot:.4f} sample start {buf[5] / tot:.4f} (wave cycles {tot})")
    print(f"refill rounds {rounds} lanes {lanes} mean lanes {mean:.2f} of 64")
    print(f"projection: ({share:.4f}) x (1 - {mean:.2f} / 64) = {share * (1.0 - mean / 64.0):.4f} of the wave cycles",
          flush=True)
    # the main loop's shade passes by whether the iteration skipped the walk (camera-only passes): passes, mean
    # lanes, and the share of the wave cycles that phases 4, 6 and 7 take inside the skipping iterations
    s_calls, s_lanes, w_calls, w_lanes = sk[0], sk[1], sk[2], sk[3]
    s_cyc = sk[4] + sk[5] + sk[6]
    s_mean = s_lanes / s_calls if s_calls else 0.0
    w_mean = w_lanes / w_calls if w_calls else 0.0
    s_share = s_cyc / tot
    print(f"shade passes: walk skipped {s_calls} lanes {s_lanes} mean {s_mean:.2f}; walked {w_calls} lanes {w_lanes} "
          f"mean {w_mean:.2f}")
    print(f"cycles in walk-skipping iterations: shading {sk[4]} samplers {sk[5]} stores {sk[6]} "
          f"share {s_share:.4f} of the wave cycles")
    print(f"projection: {s_share:.4f} x (1 - {s_mean:.2f} / 64) = {s_share * (1.0 - s_mean / 64.0):.4f} of the wave cycles",
          flush=True)


if __name__ == "__main__":
    main()
