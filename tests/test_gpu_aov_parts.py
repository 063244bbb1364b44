"""First-hit AOV accumulators across partitions on the device (rtw_aov_create_part, rtw_aov_pack,
rtw_aov_merge_parts, rtw_aov_export_state / import_state, distributed.py).

The contract: N partition AOV accumulators, packed, gathered and merged, are bit for bit the accumulator one GPU
holds after the same adds -- every plane, the hit counts, the header and the zeros of the padding slots -- so its
albedo, normal and depth are the oracle's (tests/aov_ref.py) and every later add is the single accumulator's.
37 x 19 is 5 x 3 tiles with edge tiles on both axes: N = 4 gives parts of 4, 4, 4 and 3 tiles (lanes past the part
in the last block), N = 16 leaves part 15 without tiles.  The oracle references are computed once per world."""
import functools
import os
import socket
import time

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.aov import AovState
from raytracinginaweekend_amd.distributed import tile_slots
from tests import aov_ref as A
from tests.parity import assert_bit_identical

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, SEED, ADDS = R.Size2i(37, 19), 7, (2, 3)
SPP = sum(ADDS)
DEPTH = 50
WORLDS = ["final_scene1", "suzanne", "cornell_box_smoke", "earth_motion"]  # lists, triangles, volume draws, texture + motion


def same_state(a: AovState, b: AovState, what="") -> None:
    assert a.header() == b.header(), what
    for name in ("albedo", "normal", "depth", "hits"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.shape == y.shape and (x.view(np.uint32) == y.view(np.uint32)).all(), (what, name)


def make_parts(dw, size, n, seed=SEED, **kw):
    return [R.AovAccumulator(dw, size, seed=seed, part=(r, n), **kw) for r in range(n)]


def pack_and_merge(parts, whole, pad_bytes=0, offset_words=0, fill=-1):
    """Packs every part into one gathered device buffer and merges it into `whole`; returns (buffer, stride)."""
    import torch

    n = len(parts)
    stride = parts[0].packed_bytes() + pad_bytes
    assert all(p.packed_bytes() == parts[0].packed_bytes() for p in parts) and stride % 4 == 0
    buf = torch.full((offset_words + n * stride // 4,), fill, dtype=torch.int32, device=torch.device("cuda", whole.device))
    gathered = buf[offset_words:]
    for r, p in enumerate(parts):
        p.pack_into(gathered[r * stride // 4: (r + 1) * stride // 4])
    whole.merge_parts(gathered, stride, n)
    return buf, stride


@functools.lru_cache(maxsize=None)
def oracle_aovs(getter, name):
    """(albedo, normal, depth, hits) of the oracle at SIZE, SPP, SEED: the twin, the Normals frame, the sample loop."""
    world = getter(name)
    depth, hits = A.depth_hits(world, SIZE, SPP, SEED)
    return (A.twin_albedo(world, SIZE, SPP, SEED), O.render(world, R.render_params(SIZE, SPP, DEPTH, R.RenderMode.Normals, seed=SEED)),
            depth, hits)


@functools.lru_cache(maxsize=None)
def single_state(getter, name):
    """The state of a plain AovAccumulator after ADDS (computed once per world; the tests only read it)."""
    single = R.AovAccumulator(getter(name), SIZE, seed=SEED)
    for k in ADDS:
        single.add(k)
    st = single.state()
    single.release()
    single.dworld.release()
    return st


# ---- 1. merge equals the single accumulator; 2. a part alone ------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("name", WORLDS)
def test_merge_equals_the_single_accumulator(worlds, name, n):
    dw = R.DeviceWorld(worlds(name), 0)
    whole = R.AovAccumulator(dw, SIZE, seed=SEED)
    parts = make_parts(dw, SIZE, n)
    assert [p.tiles for p in parts] == [len(range(r, 15, n)) for r in range(n)] and whole.tiles == 15
    for k in ADDS:
        for p in parts:
            p.add(k)
    want = single_state(worlds, name)
    # a part alone: its planes are the whole accumulator's at its tiles (else the kernel is wrong, not the merge)
    for r, (p, q) in enumerate(zip(parts, want.split(n))):
        same_state(p.state(), q, f"part {r} of {n} alone")
    gathered, stride = pack_and_merge(parts, whole)
    host = gathered.cpu().numpy().view(np.uint32).reshape(n, -1)
    for r, p in enumerate(parts):  # the records: numpy's packing of the parts' exported states, word for word
        assert (host[r] == p.state().packed(stride)).all(), f"record {r}"
    assert whole.samples == SPP
    same_state(whole.state(), want, "merged state")
    albedo, normal, depth, hits = oracle_aovs(worlds, name)
    assert_bit_identical(whole.albedo(), albedo, f"{name} merged albedo against the twin")
    assert_bit_identical(whole.normal(), normal, f"{name} merged normal against the oracle's Normals frame")
    assert_bit_identical(whole.depth(), depth, f"{name} merged depth")
    assert (whole.hits() == hits).all() and hits.max() == SPP
    dw.release()


def test_more_parts_than_tiles(worlds):
    name, n = "final_scene1", 16
    dw = R.DeviceWorld(worlds(name), 0)
    whole = R.AovAccumulator(dw, SIZE, seed=SEED)
    parts = make_parts(dw, SIZE, n)
    assert [p.tiles for p in parts] == [1] * 15 + [0]
    for k in ADDS:
        for p in parts:
            p.add(k)
    assert all(p.samples == SPP for p in parts)  # the part without tiles launches nothing and still counts
    empty = parts[15].state()
    assert empty.slots == 0 and empty.hits.size == 0 and empty.samples == SPP
    pack_and_merge(parts, whole)
    same_state(whole.state(), single_state(worlds, name), "16 parts of 15 tiles")
    dw.release()


# ---- 3. lists by global tile ------------------------------------------------------------------------------
def test_leaf_lists_are_indexed_by_the_frames_tile(worlds, monkeypatch):
    """final_scene1 at 160 x 90, 3 samples, N = 3 (tiles with lists, empty lists and ties at sphere rims): merged
    with lists equals merged with RTW_PRIMARY_LISTS=0 at create, and both equal the plain accumulator."""
    world, size, n = worlds("final_scene1"), R.Size2i(160, 90), 3
    dw = R.DeviceWorld(world, 0)
    plain = R.AovAccumulator(dw, size, seed=SEED)
    listed = make_parts(dw, size, n)
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "0")
    walked = make_parts(dw, size, n)
    monkeypatch.delenv("RTW_PRIMARY_LISTS")
    for aov in [plain] + listed + walked:
        aov.add(1)
        aov.add(2)
    want = plain.state()
    for parts, what in ((listed, "lists"), (walked, "walk")):
        whole = R.AovAccumulator(dw, size, seed=SEED)
        pack_and_merge(parts, whole)
        same_state(whole.state(), want, f"merged parts ({what}) against the plain accumulator")
    dw.release()


# ---- 4. both copy widths ----------------------------------------------------------------------------------
def test_both_copy_widths_and_untouched_padding(worlds):
    name, n = "cornell_box_smoke", 3
    dw = R.DeviceWorld(worlds(name), 0)
    parts = make_parts(dw, SIZE, n)
    for k in ADDS:
        for p in parts:
            p.add(k)
    want = single_state(worlds, name)
    words = parts[0].packed_bytes() // 4
    PATTERN = 0x5A5A5A5A
    for what, kw in (("16-byte path", dict(pad_bytes=32)), ("odd stride", dict(pad_bytes=4)),
                     ("a buffer offset by 4 bytes", dict(pad_bytes=16, offset_words=1))):
        whole = R.AovAccumulator(dw, SIZE, seed=SEED)
        buf, stride = pack_and_merge(parts, whole, fill=PATTERN, **kw)
        same_state(whole.state(), want, what)
        host = buf.cpu().numpy().view(np.uint32)
        off = kw.get("offset_words", 0)
        assert (host[:off] == PATTERN).all()
        for r in range(n):  # the padding between the records is neither written by the packs nor by the merge
            rec = host[off + r * stride // 4: off + (r + 1) * stride // 4]
            assert (rec[words:] == PATTERN).all() and rec[words:].size == kw["pad_bytes"] // 4, (what, r)
            assert (rec[:words] == parts[r].state().packed()).all(), (what, r)
        whole.release()
    dw.release()


def test_an_unaligned_gather_at_an_odd_stride(worlds):
    """All channels (8 sections), 44 x 26, N = 3: the records packed into a view one word off 16 bytes and merged at
    a stride of 4 mod 16 -- only alignment keeps them off the 16-byte path -- give the bits of the aligned run."""
    size, n = R.Size2i(44, 26), 3
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    single = R.AovAccumulator(dw, size, seed=SEED)
    parts = make_parts(dw, size, n)
    for acc in parts + [single]:
        acc.add(3)
    aligned, odd = R.AovAccumulator(dw, size, seed=SEED), R.AovAccumulator(dw, size, seed=SEED)
    buf, stride = pack_and_merge(parts, aligned)
    assert buf.data_ptr() % 16 == 0 and stride % 16 == 0
    buf, stride = pack_and_merge(parts, odd, pad_bytes=4, offset_words=1)
    assert buf[1:].data_ptr() % 16 == 4 and stride % 16 == 4
    same_state(aligned.state(), single.state(), "aligned")
    same_state(odd.state(), aligned.state(), "one word off, stride 4 mod 16")
    dw.release()


# ---- 5. continue and re-partition -------------------------------------------------------------------------
def test_continue_and_repartition(worlds, tmp_path):
    name = "earth_motion"
    dw = R.DeviceWorld(worlds(name), 0)
    single = R.AovAccumulator(dw, SIZE, seed=SEED)
    three = make_parts(dw, SIZE, 3)
    for acc in three + [single]:
        acc.add(2)
    for r, p in enumerate(three):
        p.state().save(tmp_path / f"rank{r}.npz")
    merged = AovState.merge(AovState.load(tmp_path / f"rank{r}.npz") for r in range(3))
    same_state(merged, single.state(), "numpy merge of the three checkpoints")
    two = make_parts(dw, SIZE, 2)
    for acc, st in zip(two, merged.split(2)):
        acc.load_state(st)
        assert acc.samples == 2
        acc.add(3)
    whole = R.AovAccumulator(dw, SIZE, seed=SEED)
    pack_and_merge(two, whole)
    same_state(whole.state(), single_state(worlds, name), "re-partitioned 3 -> 2 and continued")
    # the merged accumulator continues too
    single.add(3)
    single.add(1)
    whole.add(1)
    same_state(whole.state(), single.state(), "the merged accumulator continues")
    dw.release()


# ---- 6. refusals ------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(worlds):
    import torch

    n = 2
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    whole = R.AovAccumulator(dw, SIZE, seed=SEED)
    whole.add(2)
    before = whole.state()
    parts = make_parts(dw, SIZE, n)
    fewer = make_parts(dw, SIZE, n, channels=("albedo", "depth"))
    for acc in parts + fewer:
        acc.add(3)
    stride = parts[0].packed_bytes()
    words = stride // 4
    good = torch.zeros(n * words, dtype=torch.int32, device="cuda:0")
    other = torch.zeros(n * words, dtype=torch.int32, device="cuda:0")
    for r in range(n):
        parts[r].pack_into(good[r * words: (r + 1) * words])
        fewer[r].pack_into(other[r * words: (r + 1) * words])  # (a smaller record inside the same stride)

    def refused(field, call, exc=N.RtwError):
        with pytest.raises(exc) as e:
            call()
        assert field in str(e.value), str(e.value)
        same_state(whole.state(), before, f"after the refusal of {field}")

    refused("part_index", lambda: parts[1].merge_parts(good, stride, n))  # a merge into a part of N > 1
    refused("channels", lambda: whole.merge_parts(other, stride, n))
    uneven = good.clone()
    uneven[words + 4] += 1  # record 1's samples
    refused("samples", lambda: whole.merge_parts(uneven, stride, n))
    refused("stride_bytes", lambda: whole.merge_parts(good, stride - 4, n))
    refused("part_index", lambda: whole.merge_parts(torch.cat([good[words:], good[:words]]), stride, n))
    colour = R.Accumulator(dw, SIZE, DEPTH, seed=SEED, part=(0, n), layout=N.LAYOUT_TILES)
    crec = torch.zeros(n * words, dtype=torch.int32, device="cuda:0")
    colour.pack_into(crec[:words])
    refused("magic", lambda: whole.merge_parts(crec, stride, n))
    # a resolve of a part: the Python face and the C entry points
    for call in (parts[0].albedo, parts[0].normal, parts[0].depth, parts[0].hits):
        refused("part", call, ValueError)
    import ctypes as C

    lib = N.lib()
    assert lib.rtw_aov_resolve(parts[0]._h, N.AOV_ALBEDO, C.c_void_p(good.data_ptr()), None) == N.RTW_ERR_UNSUPPORTED
    assert b"part_count" in lib.rtw_last_error()
    assert lib.rtw_aov_hits(parts[0]._h, C.c_void_p(good.data_ptr()), None) == N.RTW_ERR_UNSUPPORTED
    assert b"part_count" in lib.rtw_last_error()
    torch.cuda.synchronize()
    assert (good[:8].cpu().numpy() == parts[0].state().packed()[:8].view(np.int32)).all()  # nothing was written
    # import: a header of another part, a hit count above the samples, a non-zero padding slot
    own, st = parts[0].state(), parts[1].state()
    refused("part_index", lambda: parts[0].load_state(st))
    bad = parts[0].state()
    bad.hits[0] = bad.samples + 1
    refused("hits", lambda: parts[0].load_state(bad))
    bad = parts[0].state()
    pad = np.flatnonzero(tile_slots(SIZE, (8, 8), (0, n)) < 0)
    bad.normal[1, pad[0]] = 1.0
    refused("normal", lambda: parts[0].load_state(bad))
    same_state(parts[0].state(), own, "the part after its refused imports")
    whole.merge_parts(good, stride, n)  # and the good buffer is taken
    assert whole.samples == 3
    dw.release()


# ---- 7. denoise from merged accumulators --------------------------------------------------------------------
def test_denoise_from_merged_accumulators(worlds):
    import torch

    world, n = worlds("earth_mapped"), 3
    dw = R.DeviceWorld(world, 0)
    acc = R.Accumulator(dw, SIZE, DEPTH, seed=SEED, moments=True)
    aov = R.AovAccumulator(dw, SIZE, seed=SEED)
    acc.add(4)
    aov.add(8)
    want = acc.denoised(guide=aov, albedo=aov)
    whole = R.Accumulator(dw, SIZE, DEPTH, seed=SEED, moments=True)
    colour_parts = [R.Accumulator(dw, SIZE, DEPTH, seed=SEED, moments=True, part=(r, n), layout=N.LAYOUT_TILES) for r in range(n)]
    aov_whole = R.AovAccumulator(dw, SIZE, seed=SEED)
    aov_parts = make_parts(dw, SIZE, n)
    for c, a in zip(colour_parts, aov_parts):
        c.add(4)
        a.add(8)
    stride = colour_parts[0].packed_bytes()
    gathered = torch.zeros(n * stride // 4, dtype=torch.int32, device="cuda:0")
    for r, c in enumerate(colour_parts):
        c.pack_into(gathered[r * stride // 4: (r + 1) * stride // 4])
    whole.merge_parts(gathered, stride, n)
    pack_and_merge(aov_parts, aov_whole)
    assert_bit_identical(whole.denoised(guide=aov_whole, albedo=aov_whole), want, "the preview from merged accumulators")
    assert (want.view(np.uint32) != acc.image().view(np.uint32)).any()
    dw.release()


# ---- 8. two ranks, one GPU ------------------------------------------------------------------------------------
SCENE8, SIZE8 = "cornell_box", (40, 40)


def _free_port() -> int:
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    return port


def _rank(rank, world_size, port, out_dir):
    import sys

    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import torch.distributed as dist

    from raytracinginaweekend_amd.distributed import DistributedAovAccumulator

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world_size)
    try:
        dw = R.DeviceWorld(R.demo_world(SCENE8), 0)
        aov = DistributedAovAccumulator(dw, R.Size2i(*SIZE8), rank, world_size, 0, seed=SEED)
        aov.add(2)
        aov.add(3)
        whole = aov.sync()
        assert (whole is None) == (rank != 0)
        if whole is not None:
            whole.state().save(os.path.join(out_dir, "whole.npz"))
            np.save(os.path.join(out_dir, "albedo.npy"), whole.albedo())
        dist.barrier()
        aov.release()
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu(worlds, tmp_path):
    import torch.multiprocessing as mp

    single = R.AovAccumulator(worlds(SCENE8), R.Size2i(*SIZE8), seed=SEED)
    single.add(5)
    want, want_albedo = single.state(), single.albedo()
    ctx = mp.start_processes(_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, start_method="spawn", join=False)
    deadline = time.monotonic() + 120
    while not ctx.join(timeout=1):  # (raises when a child exits non-zero: no retry)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the two ranks did not finish in 120 s")
    same_state(AovState.load(tmp_path / "whole.npz"), want, "the two ranks' merged state")
    assert_bit_identical(np.load(tmp_path / "albedo.npy"), want_albedo, "the two ranks' albedo")
