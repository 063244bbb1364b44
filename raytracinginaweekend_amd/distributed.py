"""Multi-GPU frame rendering: interleaved tile partition + one collective gather.

One process per GPU (torch.distributed, backend "nccl" = RCCL over xGMI).  Rank r renders the
tiles t with t % N == r of the frame into a compact tile buffer (RTW_LAYOUT_TILES); the buffers
(padded to rank 0's size, rtw_partition_floats) are gathered onto rank 0 (one collective: RCCL's
gather is a group of point-to-point sends to rank 0 over xGMI, W*H*12/N bytes per peer) and rank 0
scatters them into the image (rtw_untile_device).  Only rank 0 holds the gather buffer and the image.  Because the RNG stream is keyed by (seed, pixel, sample), the
image is bit-identical for every N.  PyTorch is plumbing here: device memory, the stream and the
collective; the render itself is librtw.so's kernel.

TileExchange holds the partition arithmetic and the gather/untile step for both device tensors
(RCCL + the untile kernel) and host tensors (gloo + untile_host, the CPU mirror used by the
world-size-2 and -3 tests).  Reference: rendering.rs:222-252 (the reference merges per-thread planes
in one process; here the ranks own disjoint pixels, so the merge is a placement).

DistributedAccumulator is the same idea for progressive accumulators (progressive.py): every rank adds to its own
partition's accumulator, and one gather of packed state records plus one merge launch (include/rtw_parts.h) gives
rank 0 the whole image's accumulator, with its noise estimate, stop map, kept counts, denoiser and checkpoint.

DistributedAovAccumulator does the same for the first-hit AOV pass (aov.py, include/rtw_aov_parts.h): the denoiser's
guide and albedo images are traced an N-th per rank and merged on rank 0, beside the colour accumulator's state.
Both are one mechanism (_DistributedRecords): a record of another section table travels the same way.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native as N
from .rendering import DEFAULT_SEED, DeviceWorld, RenderMode, Size2i, partition_floats, render_params, untile_device
from .world import World


@dataclass
class FrameSpec:
    size: Size2i
    samples_per_pixel: int
    max_depth: int
    seed: int = 0x5EED
    tile: tuple[int, int] = (8, 8)
    thread_count: int = 1  # the reference's sample-split planes (rendering.rs:222-252)


def tile_slots(size: Size2i, tile: tuple[int, int], part: tuple[int, int]) -> np.ndarray:
    """Pixel index (or -1 for padding) of every slot of one partition's tile buffer (host-side
    mirror of the kernel's layout: owned tiles t = idx, idx + pc, ... row-major inside)."""
    tw, th = tile
    tiles_x = -(-size.width // tw)
    n_tiles = tiles_x * -(-size.height // th)
    idx, pc = part
    owned = np.arange(idx, n_tiles, pc, dtype=np.int64)[:, None]
    j = np.arange(tw * th, dtype=np.int64)[None, :]
    px = (owned % tiles_x) * tw + j % tw
    py = (owned // tiles_x) * th + j // tw
    return np.where((px < size.width) & (py < size.height), py * size.width + px, -1).ravel()


def pack_tiles(image: np.ndarray, size: Size2i, tile: tuple[int, int], part: tuple[int, int], stride: int) -> np.ndarray:
    """A partition's tile buffer (RTW_LAYOUT_TILES, padded to `stride` floats) cut from a full
    (H*W, 3) image: what the kernel writes for that partition."""
    slots = tile_slots(size, tile, part)
    buf = np.zeros(stride, np.float32)
    v = buf[: len(slots) * 3].reshape(-1, 3)
    ok = slots >= 0
    v[ok] = image.reshape(-1, 3)[slots[ok]]
    return buf


def untile_host(gathered: np.ndarray, size: Size2i, tile: tuple[int, int], part_count: int, stride: int) -> np.ndarray:
    """CPU mirror of untile_kernel (rtw_device.hip): the gathered buffers -> (H*W, 3) image."""
    img = np.zeros((size.width * size.height, 3), np.float32)
    for r in range(part_count):
        slots = tile_slots(size, tile, (r, part_count))
        src = gathered[r * stride: r * stride + len(slots) * 3].reshape(-1, 3)
        ok = slots >= 0
        img[slots[ok]] = src[ok]
    return img


class TileExchange:
    """Partition arithmetic + the gather step of one frame for rank `rank` of `world_size`."""

    def __init__(self, spec: FrameSpec, rank: int, world_size: int):
        self.spec, self.rank, self.world_size = spec, rank, world_size
        p0 = render_params(spec.size, 1, 1, tile=spec.tile, part=(0, world_size), layout=N.LAYOUT_TILES)
        self.stride = partition_floats(p0)  # rank 0 owns the most tiles
        self.params = render_params(spec.size, spec.samples_per_pixel, spec.max_depth, seed=spec.seed,
                                    tile=spec.tile, part=(rank, world_size),
                                    layout=N.LAYOUT_TILES if world_size > 1 else N.LAYOUT_IMAGE,
                                    thread_count=spec.thread_count)

    def pixels_this_rank(self) -> int:
        return int((tile_slots(self.spec.size, self.spec.tile, (self.rank, self.world_size)) >= 0).sum())

    def gather(self, tiles, gathered=None) -> None:
        """Gather the padded tile buffers onto rank 0 (RCCL for device tensors, gloo for host ones):
        rank r's buffer lands at gathered[r * stride : (r + 1) * stride] of rank 0's `gathered`;
        other ranks pass None (they send only)."""
        import torch.distributed as dist

        if self.rank == 0:
            parts = list(gathered.view(self.world_size, -1).unbind(0))
            dist.gather(tiles, parts, dst=0)
        else:
            dist.gather(tiles, None, dst=0)

    def untile(self, gathered, image, stream_ptr: int | None = None) -> None:
        """Rank 0: scatter the gathered buffers into the (W*H*3) image."""
        if gathered.is_cuda:
            untile_device(self.params, gathered.data_ptr(), self.stride, image.data_ptr(), stream_ptr)
        else:
            import torch

            img = untile_host(gathered.numpy(), self.spec.size, self.spec.tile, self.world_size, self.stride)
            image.copy_(torch.from_numpy(img.ravel()))


class FrameRenderer:
    """Renders frames of one World on `device` as rank `rank` of `world_size`."""

    def __init__(self, world: World, spec: FrameSpec, rank: int = 0, world_size: int = 1, device: int = 0):
        import torch

        self.torch = torch
        self.spec, self.rank, self.world_size = spec, rank, world_size
        self.dev = torch.device("cuda", device)
        self.dworld = DeviceWorld(world, device)
        self.xchg = TileExchange(spec, rank, world_size)
        self.params = self.xchg.params
        self.stride = self.xchg.stride
        npix = spec.size.width * spec.size.height
        self.image = torch.zeros(npix * 3, dtype=torch.float32, device=self.dev)
        if world_size > 1:
            self.tiles = torch.zeros(self.stride, dtype=torch.float32, device=self.dev)
            self.gathered = (torch.zeros(self.stride * world_size, dtype=torch.float32, device=self.dev)
                             if rank == 0 else None)

    def stream_ptr(self) -> int:
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def launch(self) -> None:
        """The render kernel alone (asynchronous, on the current stream)."""
        out = self.image if self.world_size == 1 else self.tiles
        self.dworld.render_into(self.params, out.data_ptr(), self.stream_ptr())

    def exchange(self) -> None:
        """One RCCL gather of the tile buffers onto rank 0 + the untile there."""
        if self.world_size == 1:
            return
        self.xchg.gather(self.tiles, self.gathered)
        if self.rank == 0:
            self.xchg.untile(self.gathered, self.image, self.stream_ptr())

    def render_frame(self):
        self.launch()
        self.exchange()
        return self.image

    def pixels_this_rank(self) -> int:
        return self.xchg.pixels_this_rank()


def gather_records(record, gathered, rank: int, world_size: int) -> None:
    """The accumulators' one collective: every rank's packed record (progressive.py; all of one size) onto rank 0,
    rank r's at gathered[r * len(record):] there; other ranks pass None.  Device tensors with RCCL, host tensors
    with gloo, as `TileExchange.gather`."""
    import torch.distributed as dist

    if rank == 0:
        dist.gather(record, list(gathered.view(world_size, -1).unbind(0)), dst=0)
    else:
        dist.gather(record, None, dst=0)


class _DistributedRecords:
    """What the accumulators across ranks share: `local`, this rank's accumulator of part (rank, world_size); `whole`,
    rank 0's of the whole image (world_size 1: the same one); the record, its stride and rank 0's gathered buffer;
    `sync`.  `make(dworld, part)` builds an accumulator with `packed_bytes`, `pack_into`, `merge_parts` and
    `release`, of `part` or, for None, of the whole image."""

    def __init__(self, world: World | DeviceWorld, rank: int, world_size: int, device: int, make):
        import torch

        if not 0 <= rank < world_size:
            raise ValueError("rank must be within 0 .. world_size - 1")
        self.torch = torch
        self.rank, self.world_size = rank, world_size
        self.dev = torch.device("cuda", device)
        self.dworld = world if isinstance(world, DeviceWorld) else DeviceWorld(world, device)
        self.whole = make(self.dworld, None) if rank == 0 else None
        if world_size == 1:
            self.local = self.whole
        else:
            self.local = make(self.dworld, (rank, world_size))
            # (a stride of whole 16 bytes: every record of the gathered buffer takes the merge's 16-byte path)
            self.stride_bytes = -(-self.local.packed_bytes() // 16) * 16
            self.record = torch.zeros(self.stride_bytes // 4, dtype=torch.int32, device=self.dev)
            self.gathered = (torch.zeros(world_size * self.stride_bytes // 4, dtype=torch.int32, device=self.dev)
                             if rank == 0 else None)
        self.samples = 0

    def release(self) -> None:
        for a in {id(a): a for a in (self.local, self.whole) if a is not None}.values():
            a.release()
        self.local = self.whole = None

    def _stream(self) -> int:
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def _device_collectives(self) -> bool:
        import torch.distributed as dist

        return dist.get_backend() == "nccl"

    def sync(self):
        """Pack, one gather onto rank 0, merge: returns `whole` on rank 0 and None elsewhere.  Every rank calls it."""
        if self.world_size == 1:
            return self.whole
        self.local.pack_into(self.record, self._stream())
        if self._device_collectives():
            gather_records(self.record, self.gathered, self.rank, self.world_size)
        else:  # stage through the host on both sides
            host = self.record.cpu()
            staged = self.torch.zeros(self.gathered.numel(), dtype=self.torch.int32) if self.rank == 0 else None
            gather_records(host, staged, self.rank, self.world_size)
            if self.rank == 0:
                self.gathered.copy_(staged)
        if self.rank != 0:
            return None
        self.whole.merge_parts(self.gathered, self.stride_bytes, self.world_size, self._stream())
        return self.whole


class DistributedAccumulator(_DistributedRecords):
    """A progressive accumulator of one frame across the ranks of a process group (one process per GPU).

    Rank r owns an `Accumulator` of part (r, world_size) in LAYOUT_TILES (`local`); rank 0 also owns `whole`, a
    plain `Accumulator` of part (0, 1) on the same `DeviceWorld`.  `add` is local and asynchronous; `adapt` is the
    local decision plus one all_reduce of the two counts (the decisions are per tile, so they are one GPU's);
    `sync` packs every rank's state, gathers the records onto rank 0 with one collective and merges them into
    `whole`, which then is, bit for bit, the accumulator one GPU would hold after the same calls: read it through
    its own API (`image`, `stderr`, `noise`, `sample_counts`, `kept_counts`, `clamped_counts`, `clamp_loss`, `tile_stops`, `denoised`, `state`).
    With the nccl backend the device tensors are gathered; with any other (gloo) the record is staged through a
    host tensor on both sides, which also lets several ranks share one GPU.  world_size 1 is a pass-through
    without a collective: `local` is `whole`.

    `sync` may be called any number of times; adds after it continue the partitions (not `whole`)."""

    def __init__(self, world: World | DeviceWorld, size: Size2i, max_depth: int, rank: int = 0, world_size: int = 1,
                 device: int = 0, *, seed: int = DEFAULT_SEED, tile: tuple[int, int] = (8, 8), moments: bool = False,
                 adaptive: bool = False, finite: bool = False, render_mode: RenderMode = RenderMode.Default,
                 clamp: float | None = None):
        from .progressive import Accumulator

        kw = dict(seed=seed, device=device, tile=tile, moments=moments, adaptive=adaptive, finite=finite, clamp=clamp)

        def make(dworld, part):
            if part is None:
                return Accumulator(dworld, size, max_depth, render_mode, **kw)
            return Accumulator(dworld, size, max_depth, render_mode, part=part, layout=N.LAYOUT_TILES, **kw)

        super().__init__(world, rank, world_size, device, make)
        tw, th = tile
        self.frame_tiles = -(-size.width // tw) * -(-size.height // th)
        self.adaptive = bool(adaptive)
        # (samples: the group's frontier, the samples of the active tiles, as one GPU would count them)
        self.active_tiles = self.frame_tiles

    def add(self, n: int) -> None:
        """The next `n` samples of this rank's pixels (asynchronous; adaptive: of its active tiles).  Like one
        GPU's accumulator, an adaptive group whose tiles have all stopped adds nothing and does not count."""
        if n < 0:
            raise ValueError("n must be >= 0")
        if self.adaptive and self.active_tiles == 0:
            return
        self.local.add(n, self._stream())
        self.samples += n

    def adapt(self, target: float, min_samples: int = 16) -> tuple[int, int]:
        """`Accumulator.adapt` on this rank's tiles, then one all_reduce(SUM): (active tiles, active pixels) of the
        group.  Every rank calls it."""
        # (a rank without tiles, or one whose tiles stopped before, holds fewer samples than the stop test asks
        # for only in the first case: it has nothing to decide)
        t, p = self.local.adapt(target, min_samples, self._stream()) if self.local.tiles > 0 else (0, 0)
        if self.world_size > 1:
            import torch.distributed as dist

            counts = self.torch.tensor([t, p], dtype=self.torch.int64, device=self.dev if self._device_collectives() else "cpu")
            dist.all_reduce(counts, op=dist.ReduceOp.SUM)
            t, p = (int(v) for v in counts.tolist())
        self.active_tiles = t
        return t, p


class DistributedAovAccumulator(_DistributedRecords):
    """The first-hit AOV accumulator of one frame across the ranks of a process group (one process per GPU): the
    guide and albedo images of `DistributedAccumulator`'s denoised preview, traced an N-th per rank.

    Rank r owns an `AovAccumulator` of part (r, world_size) (`local`); rank 0 also owns `whole`, a plain
    `AovAccumulator` on the same `DeviceWorld`.  `add` is local and asynchronous; `sync` packs every rank's planes,
    gathers the records onto rank 0 with one collective and merges them into `whole`, which then is, bit for bit,
    the accumulator one GPU would hold after the same adds: resolve it, or hand it to `Accumulator.denoised`.
    With the nccl backend the device tensors are gathered; with any other (gloo) the record is staged through a
    host tensor on both sides, which also lets several ranks share one GPU.  world_size 1 is a pass-through
    without a collective: `local` is `whole`.  Pass the `DeviceWorld` of the colour accumulator to share its
    resident world.

    `sync` may be called any number of times; adds after it continue the partitions (not `whole`)."""

    def __init__(self, world: World | DeviceWorld, size: Size2i, rank: int = 0, world_size: int = 1, device: int = 0, *,
                 seed: int = DEFAULT_SEED, channels=("albedo", "normal", "depth")):
        from .aov import AovAccumulator

        def make(dworld, part):
            return AovAccumulator(dworld, size, seed=seed, device=device, channels=channels, part=part or (0, 1))

        super().__init__(world, rank, world_size, device, make)

    def add(self, n: int) -> None:
        """The next `n` camera samples of this rank's pixels (asynchronous)."""
        if n < 0:
            raise ValueError("n must be >= 0")
        self.local.add(n, self._stream())
        self.samples += n


def render_adaptive_distributed(world: World | DeviceWorld, size: Size2i, max_depth: int, rank: int, world_size: int,
                                device: int, target: float, max_samples: int, min_samples: int = 16, batch: int = 16, **kw):
    """`render_adaptive` across a process group: add and adapt until the group has no active tile or the frontier
    reaches `max_samples`, then one `sync`.  Rank 0 returns (image, sample_counts, info) as `render_adaptive` does,
    bit for bit its values; the other ranks return None.  Keyword arguments go to `DistributedAccumulator`."""
    if max_samples < 2 or batch < 1 or min_samples < 2:
        raise ValueError("max_samples and min_samples must be >= 2 and batch >= 1")
    kw["adaptive"] = True
    acc = DistributedAccumulator(world, size, max_depth, rank, world_size, device, **kw)
    try:
        active = acc.frame_tiles
        while active > 0 and acc.samples < max_samples:
            acc.add(min(batch, max_samples - acc.samples))
            if acc.samples >= min_samples:
                active = acc.adapt(target, min_samples)[0]
        whole = acc.sync()
        if whole is None:
            return None
        counts = whole.sample_counts()
        info = {"samples": whole.samples, "samples_rendered": int(counts.astype(np.int64).sum()), "active_tiles": active,
                "noise": whole.noise()[0]}
        return whole.image(), counts, info
    finally:
        acc.release()
