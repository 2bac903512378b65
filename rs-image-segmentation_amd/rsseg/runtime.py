"""
Host runtime over the C ABI: one Context per process / GPU.

torch-ROCm is used for three things only: device allocations (tensors as buffers, `.data_ptr()`
handed to the library), the current HIP stream, and `torch.distributed` (backend "nccl" = RCCL over
xGMI) behind the library's all-reduce hook.  All arithmetic on rasters happens in librsseg_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L


class RssegError(RuntimeError):
    pass


class RssegUnsupported(RssegError):
    """RSSEG_ERR_UNSUPPORTED: a valid input beyond a capacity of the kernels (more than 64 features / classes, ...).
    Never swallowed by the mirrors: the reference would have produced a result, so an all-zero map would be a lie."""


def _torch():
    import torch
    return torch


class CompactPlan:
    """What Context.compact_plan returns and compact / expand take: the mask (flat uint8 device tensor), its tile offsets
    (device int64, ceil(n / tile) + 1 entries, the plan's own memory), the pixel count n and the valid count n_valid."""
    __slots__ = ("mask", "tile_off", "n", "n_valid")

    def __init__(self, mask, tile_off, n: int, n_valid: int):
        self.mask, self.tile_off, self.n, self.n_valid = mask, tile_off, int(n), int(n_valid)


def make_allreduce_hook(buf, group=None, stream=None):
    """The Python side of rsseg_allreduce_fn: reduces `count` elements of `dtype` at byte `offset` of the
    communication buffer `buf` (a uint8 tensor; on the GPU in production, so the collective is RCCL over
    xGMI; a CPU tensor with the gloo backend in the CPU tests) in place across the ranks of `group`.

    Stream contract (include/rsseg.h): the collective is ordered after the work already enqueued on the context's
    stream and its result is visible to work enqueued there afterwards.  torch.distributed gives exactly that for the
    CURRENT stream (ProcessGroupNCCL makes its communication stream wait for the current stream, and a synchronous
    collective makes the current stream wait for the communication stream — no host synchronisation), so the hook
    runs the collective with the context's stream current and does not block the host: the library pays one
    hipStreamSynchronize per collective, after its copy-back.  Backends other than RCCL (gloo rehearsals on a CUDA
    buffer) are followed by a stream synchronisation, since their stream semantics are not relied on."""
    torch = _torch()
    import torch.distributed as dist
    views = {L.F32: torch.float32, L.F64: torch.float64, L.I64: torch.int64}
    ops = {L.SUM: dist.ReduceOp.SUM, L.MIN: dist.ReduceOp.MIN, L.MAX: dist.ReduceOp.MAX}
    is_nccl = buf.is_cuda and dist.get_backend(group) == "nccl"

    def hook(_user, offset, count, dtype, op):
        try:
            esz = 4 if dtype == L.F32 else 8
            t = buf[offset:offset + count * esz].view(views[dtype])
            if buf.is_cuda and stream is not None:
                with torch.cuda.stream(stream):
                    dist.all_reduce(t, op=ops[op], group=group)
                    if not is_nccl:
                        stream.synchronize()
            else:
                dist.all_reduce(t, op=ops[op], group=group)
                if buf.is_cuda and not is_nccl:
                    torch.cuda.current_stream().synchronize()
            return 0
        except Exception as e:  # noqa: BLE001 — must not propagate through the C frame
            print(f"[rsseg] all-reduce hook failed: {e!r}", flush=True)
            return 1

    return hook


class Context:
    """Owns an rsseg_ctx.  `group` (optional) is a torch.distributed process group: when its world
    size is > 1 the library's reductions go through RCCL (or gloo in CPU tests of the hook)."""

    def __init__(self, device: int = 0, group=None, use_dist: Optional[bool] = None, stream=None, force_comm: bool = False,
                 comm: Optional[str] = None):
        """stream: a torch.cuda.Stream for this context (default: torch's current stream).
        force_comm: install the all-reduce path even when the group has ONE rank (identity reductions), so that every
        collective of a step runs through the backend — the way to exercise the RCCL path on a one-GPU box.
        comm: 'native' — the library drives RCCL itself (rsseg_ctx_set_comm_rccl: its own communicator, ncclAllReduce on the
        context's stream, no Python in the loop; torch.distributed only carries the 128-byte unique id once); 'torch' — the
        callback into torch.distributed.all_reduce.  Default ($RSSEG_COMM overrides): 'native' when the group's backend is
        nccl (= RCCL), 'torch' otherwise (gloo rehearsals)."""
        torch = _torch()
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise RssegError("no GPU visible to torch: the rsseg product path needs an MI355X (no CPU fallback)")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        self.torch_stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        # torch's default stream is the legacy null stream (handle 0).  NULL would make the library create a private
        # non-blocking stream that does NOT order after torch kernels still writing an input plane, so the legacy
        # default stream is named explicitly (hipStreamLegacy == (hipStream_t)1).
        handle = self.torch_stream.cuda_stream or 1
        rc = self.lib.rsseg_ctx_create(device, C.c_void_p(handle), C.byref(h))
        if rc != 0:
            raise RssegError(f"rsseg_ctx_create failed ({rc}): {self.lib.rsseg_last_error(None).decode()}")
        self.h = h
        self.rank, self.world = 0, 1
        self._comm_buf = None
        self._hook = None
        import torch.distributed as dist
        if use_dist is None:
            use_dist = dist.is_available() and dist.is_initialized()
        if force_comm and not use_dist:
            raise RssegError("force_comm needs an initialised torch.distributed process group")
        self.comm_kind = None
        if use_dist and (dist.get_world_size(group) > 1 or force_comm):
            kind = comm or os.environ.get("RSSEG_COMM") or ("native" if dist.get_backend(group) == "nccl" else "torch")
            if kind == "native-only":
                kind = "native"
            if kind not in ("native", "torch"):
                raise ValueError(f"comm={kind!r}: 'native' or 'torch'")
            if kind == "native":
                try:
                    self._install_comm_rccl(group)
                except (RssegError, OSError) as e:
                    # a failure every rank meets alike (librccl not loadable, a symbol missing, ncclCommInitRank refusing the
                    # topology): fall back to the callback provider LOUDLY rather than lose the run; RSSEG_COMM=native-only forbids it
                    if os.environ.get("RSSEG_COMM") == "native-only" or comm == "native":
                        raise
                    print(f"[rsseg] native RCCL provider unavailable ({e}); using the torch.distributed callback", flush=True)
                    kind = "torch"
                    self._install_comm(group)
            else:
                self._install_comm(group)
            self.comm_kind = kind

    # ---- communication hook ----------------------------------------------------------------
    def _install_comm(self, group):
        torch = _torch()
        import torch.distributed as dist
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self._comm_buf = torch.zeros(1 << 22, dtype=torch.uint8, device=self.device)
        self._hook = L.ALLREDUCE_FN(make_allreduce_hook(self._comm_buf, group, self.torch_stream))
        self._chk(self.lib.rsseg_ctx_set_comm(self.h, self.rank, self.world, self._hook, None,
                                              C.c_void_p(self._comm_buf.data_ptr()), self._comm_buf.numel()))

    def _install_comm_rccl(self, group):
        """RCCL driven from C: rank 0 makes the ncclUniqueId, torch.distributed hands its 128 bytes to the other ranks (the
        only use of the process group), every rank joins the library's own communicator."""
        torch = _torch()
        import torch.distributed as dist
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        cpath = path.encode() if os.path.exists(path) else None
        box = [None]
        if self.rank == 0:
            raw = (C.c_char * 128)()
            rc = self.lib.rsseg_rccl_unique_id(cpath, C.cast(raw, C.c_void_p))
            # a failure here travels to every rank in place of the id, so that all of them take the same decision
            box[0] = bytes(raw.raw) if rc == 0 else f"rsseg_rccl_unique_id failed ({rc}): {self.lib.rsseg_last_error(None).decode()}"
        if self.world > 1:
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        if not isinstance(box[0], bytes):
            raise RssegError(str(box[0]))
        uid = (C.c_char * 128).from_buffer_copy(box[0])
        self._comm_buf = torch.zeros(1 << 22, dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        self._chk(self.lib.rsseg_ctx_set_comm_rccl(self.h, self.rank, self.world, C.cast(uid, C.c_void_p), cpath,
                                                   C.c_void_p(self._comm_buf.data_ptr()), self._comm_buf.numel()))

    def allreduce(self, offset: int, count: int, dtype: int, op: int):
        """One in-place reduction of `count` elements at byte `offset` of the communication buffer (self._comm_buf) over the
        installed path, enqueued on this context's stream (rsseg_ctx_allreduce)."""
        self._chk(self.lib.rsseg_ctx_allreduce(self.h, offset, count, dtype, op))

    def install_comm_hook(self, rank: int, world: int, hook):
        """A caller-supplied all-reduce instead of torch.distributed: hook(buf, offset, count, dtype, op) -> None reduces
        `count` elements of `dtype` (rsseg._lib F32 / F64 / I64) at byte `offset` of the uint8 device tensor `buf` in place
        across the caller's ranks, ordered after the work on this context's stream (rsseg_allreduce_fn's contract).  Used
        by the test-suite to run many ranks as threads of one process on one GPU."""
        torch = _torch()
        self.rank, self.world = int(rank), int(world)
        self._comm_buf = torch.zeros(1 << 22, dtype=torch.uint8, device=self.device)
        buf = self._comm_buf

        def cb(_user, offset, count, dtype, op):
            try:
                hook(buf, offset, count, dtype, op)
                return 0
            except Exception as e:  # noqa: BLE001 — must not propagate through the C frame
                print(f"[rsseg] all-reduce hook failed: {e!r}", flush=True)
                return 1

        self._hook = L.ALLREDUCE_FN(cb)
        self._chk(self.lib.rsseg_ctx_set_comm(self.h, self.rank, self.world, self._hook, None,
                                              C.c_void_p(self._comm_buf.data_ptr()), self._comm_buf.numel()))

    def _needs_keep(self) -> bool:
        """A temporary dropped by Python goes back to torch's caching allocator, which reuses it in the order of the stream
        it was ALLOCATED on (torch's current stream).  When that is this context's stream — the default — queued kernels
        that still read the block run before anything that could overwrite it, so nothing has to be kept alive and the
        pipelines free their temporaries as they go (keeping everything until end_async() raised the peak by
        several planes).  Only a context on a side stream (aux()), or one that has handed work to such a stream, must hold on to them until sync()."""
        if not getattr(self, "_async", False):
            return False
        if getattr(self, "_aux", None) is not None:
            return True     # a second stream allocates from the same pool: a block freed here could be rewritten there too early
        return self.torch_stream != _torch().cuda.current_stream(self.device)

    def set_async(self, on: bool = True):
        """Asynchronous entry points.  On a side stream, buffers handed out by empty() are kept alive until sync(): the
        caching allocator would otherwise recycle a temporary the moment Python drops it, while kernels that
        read it are still queued on this context's stream (_needs_keep)."""
        self._chk(self.lib.rsseg_ctx_set_async(self.h, int(on)))
        self._async = bool(on)
        self._keep = []

    def sync(self):
        self._chk(self.lib.rsseg_ctx_sync(self.h))
        self._keep = []

    def end_async(self):
        """Back to synchronous entry points.  The buffers kept alive for queued kernels are released to torch's caching
        allocator, which recycles them in stream order: safe when this context's stream is the stream they were allocated
        on (torch's current stream, the default); a context on a side stream (aux()) must use sync() instead."""
        self._chk(self.lib.rsseg_ctx_set_async(self.h, 0))
        self._async = False
        if self.torch_stream != _torch().cuda.current_stream(self.device):
            self._chk(self.lib.rsseg_ctx_sync(self.h))
        self._keep = []

    def aux(self):
        """A second context on its own HIP stream (same device, asynchronous entry points): lets a
        VALU-bound kernel run beside the HBM-bound passes issued through this context."""
        if getattr(self, "_aux", None) is None:
            torch = _torch()
            a = Context(self.device.index, use_dist=False, stream=torch.cuda.Stream(self.device))
            a.set_async(True)
            self._aux = a
        return self._aux

    def close(self):
        if getattr(self, "_aux", None) is not None:
            self._aux.close()
            self._aux = None
        if getattr(self, "h", None):
            self.lib.rsseg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _chk(self, rc: int):
        if rc != 0:
            msg = self.lib.rsseg_last_error(self.h).decode(errors="replace")
            if rc == -1:
                raise ValueError(msg)
            if rc == -3:
                raise MemoryError(msg)
            if rc == -5:
                raise RssegUnsupported(msg)
            raise RssegError(f"rsseg error {rc}: {msg}")

    # ---- buffers --------------------------------------------------------------------------------
    def to_device(self, a: np.ndarray, dtype=None):
        torch = _torch()
        a = np.ascontiguousarray(a, dtype=dtype)
        return torch.from_numpy(a).to(self.device)

    def upload_f32(self, a: np.ndarray):
        """A band as a flat float32 device plane — the reference's `.astype(np.float32)` (extract.py:34).  An 8-bit raster
        crosses PCIe as 1 byte per pixel and is widened on the device (exact: every uint8 is a float32)."""
        torch = _torch()
        a = np.ascontiguousarray(a).reshape(-1)
        if a.dtype == np.uint8:
            # widened by the library's own kernel, on THIS context's stream (where the kernels that read the plane are enqueued)
            with torch.cuda.stream(self.torch_stream):
                q = torch.from_numpy(a).to(self.device)
            return self.widen_u8(q)
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    def widen_u8(self, q):
        """uint8 plane -> float32 plane (exact), rsseg_u8_to_f32."""
        torch = _torch()
        out = self.empty(q.numel(), torch.float32)
        if self._needs_keep():
            self._keep.append(q)
        self._chk(self.lib.rsseg_u8_to_f32(self.h, C.c_void_p(q.data_ptr()), q.numel(), C.c_void_p(out.data_ptr())))
        return out

    def upload_band(self, a: np.ndarray):
        """A band as a flat device plane in the narrowest form the kernels take: an 8-bit raster STAYS uint8 (order
        statistics, spectral indices and PCA read 1 byte per pixel; values identical to the float32 path on the widened
        band), anything else becomes float32 like the reference's `.astype(np.float32)` (scripts/2:156)."""
        torch = _torch()
        a = np.ascontiguousarray(a).reshape(-1)
        if a.dtype == np.uint8:
            with torch.cuda.stream(self.torch_stream):
                return torch.from_numpy(a).to(self.device)
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    @staticmethod
    def _is_u8(t) -> bool:
        return t.dtype == _torch().uint8

    def empty(self, n, dtype):
        torch = _torch()
        t = torch.empty(int(n), dtype=dtype, device=self.device)
        if self._needs_keep():
            self._keep.append(t)
        return t

    @staticmethod
    def _pp(tensors: Sequence) -> "C.Array":
        arr = (C.c_void_p * len(tensors))()
        for i, t in enumerate(tensors):
            arr[i] = None if t is None else t.data_ptr()
        return arr

    # ---- extrema of produced planes -------------------------------------------------------------
    def collect_minmax(self, on: bool = True):
        """While on, spectral_indices / resize_bilinear(_rows) / pca_fit_transform tag every plane they return with
        its (min, max) — attribute `_rsseg_minmax`, NaN counted as 0 — and kmeans_fit_predict skips its MinMaxScaler
        pass when all its planes carry the tag.  The tag describes the plane as produced: do not modify a tagged plane."""
        self._chk(self.lib.rsseg_ctx_collect_minmax(self.h, int(on)))
        self._collect = bool(on)

    def _tag_minmax(self, tensors: Sequence):
        if not getattr(self, "_collect", False):
            return
        for i, t in enumerate(tensors):
            if t is None:
                continue
            mn, mx = C.c_double(0), C.c_double(0)
            self._chk(self.lib.rsseg_ctx_last_minmax(self.h, i, C.byref(mn), C.byref(mx)))
            t._rsseg_minmax = (mn.value, mx.value)

    # ---- profiling ---------------------------------------------------------------------------
    def prof_enable(self, on=True):
        self._chk(self.lib.rsseg_prof_enable(self.h, int(on)))

    def prof_reset(self):
        self._chk(self.lib.rsseg_prof_reset(self.h))

    def host_syncs(self, reset: bool = False) -> int:
        """How often the library made the host wait for this context's stream since the last reset."""
        n = C.c_int64(0)
        self._chk(self.lib.rsseg_ctx_host_syncs(self.h, int(reset), C.byref(n)))
        return n.value

    def prof_get(self, name: str) -> Tuple[float, int]:
        ms, cnt = C.c_double(0), C.c_int64(0)
        self._chk(self.lib.rsseg_prof_get(self.h, name.encode(), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    # ---- K1 ------------------------------------------------------------------------------------
    def order_stats(self, plane, ranks: Sequence[int]) -> Tuple[np.ndarray, int]:
        if self._is_u8(plane):
            v, nn = self.order_stats_multi([plane], [list(ranks)])
            return v[0], int(nn[0])
        r = (C.c_int64 * len(ranks))(*[int(x) for x in ranks])
        out = (C.c_float * len(ranks))()
        nn = C.c_int64(0)
        self._chk(self.lib.rsseg_order_stats_f32(self.h, C.c_void_p(plane.data_ptr()), plane.numel(), r, len(ranks), out,
                                                 C.byref(nn)))
        return np.array(out[:], dtype=np.float32), nn.value

    def order_stats_multi(self, planes: Sequence, ranks: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
        """Order statistics of several planes of equal length in one call (<= 8 planes, the same number of ranks for
        each): (values [P, R] float32, n_nan [P])."""
        P, R = len(planes), len(ranks[0])
        if any(len(r) != R for r in ranks) or any(p.numel() != planes[0].numel() for p in planes):
            raise ValueError("order_stats_multi: planes / rank lists of unequal length")
        flat = (C.c_int64 * (P * R))(*[int(x) for r in ranks for x in r])
        out = (C.c_float * (P * R))()
        nn = (C.c_int64 * P)()
        if any(self._is_u8(p) for p in planes):
            if not all(self._is_u8(p) for p in planes):
                raise ValueError("order_stats_multi: uint8 and float32 planes cannot be mixed in one call")
            self._chk(self.lib.rsseg_order_stats_multi_u8(self.h, self._pp(planes), P, planes[0].numel(), flat, R, out, nn))
        else:
            self._chk(self.lib.rsseg_order_stats_multi_f32(self.h, self._pp(planes), P, planes[0].numel(), flat, R, out, nn))
        return np.array(out[:], dtype=np.float32).reshape(P, R), np.array(nn[:], dtype=np.int64)

    # ---- K2 ------------------------------------------------------------------------------------
    def normalize(self, plane, lo: float, hi: float, out=None):
        torch = _torch()
        if self._is_u8(plane):   # only the striped / NaN side paths normalise a raw band on its own: widen it first
            plane = self.widen_u8(plane)
        out = self.empty(plane.numel(), plane.dtype) if out is None else out
        self._chk(self.lib.rsseg_normalize_f32(self.h, C.c_void_p(plane.data_ptr()), plane.numel(), C.c_float(lo),
                                               C.c_float(hi), C.c_void_p(out.data_ptr())))
        return out

    def spectral_indices(self, bands5: Sequence, lohi: Optional[np.ndarray], want_norm: Sequence[bool] = (False,) * 5,
                         want: Sequence[bool] = (True,) * 7, evi_coef: Optional[Sequence[float]] = None):
        torch = _torch()
        n = bands5[0].numel()
        outs = [self.empty(n, torch.float32) if w else None for w in want]
        norms = [self.empty(n, torch.float32) if w else None for w in want_norm]
        lh = None
        if lohi is not None:
            lh = (C.c_float * 10)(*[float(v) for v in np.asarray(lohi, np.float32).reshape(-1)])
        ec = None if evi_coef is None else (C.c_float * 4)(*[float(np.float32(v)) for v in evi_coef])   # {L, C1, C2, G}
        u8 = [self._is_u8(b) for b in bands5]
        if any(u8) and not all(u8):
            raise ValueError("spectral_indices: uint8 and float32 bands cannot be mixed")
        fn = self.lib.rsseg_spectral_indices_evi_u8 if all(u8) else self.lib.rsseg_spectral_indices_evi_f32
        self._chk(fn(self.h, self._pp(bands5), n, lh, self._pp(outs), self._pp(norms), ec))
        self._tag_minmax(outs)
        return outs, norms

    def quantize_u8(self, plane, mult: float):
        torch = _torch()
        q = self.empty(plane.numel(), torch.uint8)
        self._chk(self.lib.rsseg_quantize_u8(self.h, C.c_void_p(plane.data_ptr()), plane.numel(), C.c_float(mult),
                                             C.c_void_p(q.data_ptr())))
        return q

    def normalize_quantize_u8(self, plane, lo: float, hi: float, mult: float):
        """trunc(robust_normalize(plane; lo, hi) * mult) as uint8 in one pass."""
        torch = _torch()
        q = self.empty(plane.numel(), torch.uint8)
        self._chk(self.lib.rsseg_normalize_quantize_u8(self.h, C.c_void_p(plane.data_ptr()), plane.numel(), C.c_float(lo), C.c_float(hi),
                                                       C.c_float(mult), C.c_void_p(q.data_ptr())))
        return q

    def u8_to_unit(self, q):
        torch = _torch()
        out = self.empty(q.numel(), torch.float32)
        self._chk(self.lib.rsseg_u8_to_unit_f32(self.h, C.c_void_p(q.data_ptr()), q.numel(), C.c_void_p(out.data_ptr())))
        return out

    # ---- K3 ------------------------------------------------------------------------------------
    def pca_fit_transform(self, bands: Sequence, center: Optional[np.ndarray], scale: Optional[np.ndarray],
                          n_components: int, lohi: Optional[np.ndarray] = None, fit: Optional[Tuple[int, int]] = None):
        """lohi (nb x 2 float32, optional): the bands are RAW and are robust-normalised with these percentiles on the fly.
        fit=(offset, count) (optional): fit on that pixel range of the planes only, project all of them (stripe + halo rows)."""
        torch = _torch()
        nb, n = len(bands), bands[0].numel()
        outs = [self.empty(n, torch.float32) for _ in range(n_components)]
        comp = np.zeros((n_components, nb), np.float32)
        ratio = np.zeros(n_components, np.float32)
        mean = np.zeros(nb, np.float32)
        ev = np.zeros(n_components, np.float32)
        fp = C.POINTER(C.c_float)
        cptr = None if center is None else np.ascontiguousarray(center, np.float32).ctypes.data_as(fp)
        sc64 = None if scale is None else np.ascontiguousarray(scale, np.float64)
        sptr = None if sc64 is None else sc64.ctypes.data_as(C.POINTER(C.c_double))
        lh = None
        if lohi is not None:
            lh = np.ascontiguousarray(lohi, np.float32).reshape(-1)
            if lh.size != 2 * nb:
                raise ValueError("pca_fit_transform: lohi must hold (lo, hi) for every band")
        u8 = [self._is_u8(b) for b in bands]
        if any(u8) and not all(u8):
            raise ValueError("pca_fit_transform: uint8 and float32 bands cannot be mixed")
        if all(u8):
            f0, fn_ = (0, n) if fit is None else (int(fit[0]), int(fit[1]))
            self._chk(self.lib.rsseg_pca_fit_transform_ext_u8(self.h, self._pp(bands), nb, n, f0, fn_,
                                                              None if lh is None else lh.ctypes.data_as(fp), cptr, sptr, n_components,
                                                              self._pp(outs), comp.ctypes.data_as(fp), ratio.ctypes.data_as(fp),
                                                              mean.ctypes.data_as(fp), ev.ctypes.data_as(fp)))
        elif fit is not None:
            self._chk(self.lib.rsseg_pca_fit_transform_ext_f32(self.h, self._pp(bands), nb, n, int(fit[0]), int(fit[1]),
                                                               None if lh is None else lh.ctypes.data_as(fp), cptr, sptr, n_components,
                                                               self._pp(outs), comp.ctypes.data_as(fp), ratio.ctypes.data_as(fp),
                                                               mean.ctypes.data_as(fp), ev.ctypes.data_as(fp)))
        elif lohi is None:
            self._chk(self.lib.rsseg_pca_fit_transform_f32(self.h, self._pp(bands), nb, n, cptr, sptr, n_components,
                                                           self._pp(outs), comp.ctypes.data_as(fp), ratio.ctypes.data_as(fp),
                                                           mean.ctypes.data_as(fp), ev.ctypes.data_as(fp)))
        else:
            self._chk(self.lib.rsseg_pca_fit_transform_raw_f32(self.h, self._pp(bands), nb, n, lh.ctypes.data_as(fp), cptr, sptr, n_components,
                                                               self._pp(outs), comp.ctypes.data_as(fp), ratio.ctypes.data_as(fp),
                                                               mean.ctypes.data_as(fp), ev.ctypes.data_as(fp)))
        self._tag_minmax(outs)
        return outs, comp, ratio, mean, ev

    def indices_pca(self, bands: Sequence, lohi: np.ndarray, center: Optional[np.ndarray], scale: Optional[np.ndarray], n_components: int,
                    want_norm: Sequence[bool] = (False,) * 5, fit: Optional[Tuple[int, int]] = None, evi_coef: Optional[Sequence[float]] = None,
                    quantize: Optional[Tuple[float, float, float]] = None):
        """The seven spectral indices and the PCA of the same RAW bands with one pass less than spectral_indices +
        pca_fit_transform (rsseg_indices_pca_*): returns (index planes [7], normalised bands [5] (None where not wanted),
        component planes, components, ratio, mean, explained_variance) — the same bits as the two separate calls.
        quantize=(lo2, hi2, mult): additionally the uint8 plane normalize_quantize_u8(normalised NIR, lo2, hi2, mult) — the
        texture chain's input — left in `self.last_quantized`."""
        torch = _torch()
        nb, n = len(bands), bands[0].numel()
        idx = [self.empty(n, torch.float32) for _ in range(7)]
        norms = [self.empty(n, torch.float32) if w else None for w in want_norm]
        pcs = [self.empty(n, torch.float32) for _ in range(n_components)]
        comp = np.zeros((n_components, nb), np.float32)
        ratio = np.zeros(n_components, np.float32)
        mean = np.zeros(nb, np.float32)
        ev = np.zeros(n_components, np.float32)
        fp = C.POINTER(C.c_float)
        lh = np.ascontiguousarray(lohi, np.float32).reshape(-1)
        if lh.size != 2 * nb:
            raise ValueError("indices_pca: lohi must hold (lo, hi) for every band")
        cptr = None if center is None else np.ascontiguousarray(center, np.float32).ctypes.data_as(fp)
        sc64 = None if scale is None else np.ascontiguousarray(scale, np.float64)
        sptr = None if sc64 is None else sc64.ctypes.data_as(C.POINTER(C.c_double))
        ec = None if evi_coef is None else (C.c_float * 4)(*[float(np.float32(v)) for v in evi_coef])
        u8 = [self._is_u8(b) for b in bands]
        if any(u8) and not all(u8):
            raise ValueError("indices_pca: uint8 and float32 bands cannot be mixed")
        f0, fn_ = (0, n) if fit is None else (int(fit[0]), int(fit[1]))
        fn = self.lib.rsseg_indices_pca_u8 if all(u8) else self.lib.rsseg_indices_pca_f32
        q = self.empty(n, torch.uint8) if quantize is not None else None
        qlo, qhi, qm = (0.0, 1.0, 1.0) if quantize is None else [float(v) for v in quantize]
        self._chk(fn(self.h, self._pp(bands), nb, n, f0, fn_, lh.ctypes.data_as(fp), cptr, sptr, n_components, ec, self._pp(idx), self._pp(norms),
                     self._pp(pcs), None if q is None else C.c_void_p(q.data_ptr()), C.c_float(qlo), C.c_float(qhi), C.c_float(qm),
                     comp.ctypes.data_as(fp), ratio.ctypes.data_as(fp), mean.ctypes.data_as(fp), ev.ctypes.data_as(fp)))
        self._tag_minmax(idx + pcs)
        self.last_quantized = q      # the uint8 texture-chain input of this call (None unless `quantize` was given)
        return idx, norms, pcs, comp, ratio, mean, ev

    # ---- K4..K8 --------------------------------------------------------------------------------
    def glcm(self, q, H: int, W: int, levels: int, win: int, step: int, offsets=None):
        """The five GLCM property maps of the windows of q.  offsets: the (dr, dc) entries of pipeline.glcm_offset_plan in
        entry order (None: the four default angles at distance 1, rsseg_glcm_u8)."""
        torch = _torch()
        oh, ow = (H - win) // step + 1, (W - win) // step + 1
        outs = [self.empty(oh * ow, torch.float32) for _ in range(5)]
        if offsets is None:
            self._chk(self.lib.rsseg_glcm_u8(self.h, C.c_void_p(q.data_ptr()), H, W, levels, win, step, self._pp(outs)))
            return outs, (oh, ow)
        # an offset at least 2^15 long leaves every window: its sign is kept, its length clamped to fit 16 bits
        flat = [max(-32767, min(32767, int(v))) for o in offsets for v in o]
        arr = (C.c_int32 * len(flat))(*flat)
        self._chk(self.lib.rsseg_glcm_offsets_u8(self.h, C.c_void_p(q.data_ptr()), H, W, levels, win, step, arr, len(offsets),
                                                 self._pp(outs)))
        return outs, (oh, ow)

    def resize_bilinear(self, src, sh: int, sw: int, dh: int, dw: int):
        torch = _torch()
        dst = self.empty(dh * dw, torch.float32)
        self._chk(self.lib.rsseg_resize_bilinear_f32(self.h, C.c_void_p(src.data_ptr()), sh, sw, C.c_void_p(dst.data_ptr()),
                                                     dh, dw))
        self._tag_minmax([dst])
        return dst

    def resize_bilinear_rows(self, src, sh_local: int, sw: int, src_row0: int, sh: int, dh_local: int, dw: int, dst_row0: int, dh: int):
        torch = _torch()
        dst = self.empty(dh_local * dw, torch.float32)
        self._chk(self.lib.rsseg_resize_bilinear_rows_f32(self.h, C.c_void_p(src.data_ptr()), sh_local, sw, src_row0, sh,
                                                          C.c_void_p(dst.data_ptr()), dh_local, dw, dst_row0, dh))
        self._tag_minmax([dst])
        return dst

    # The window operators take `rows=(y0, y1)` and `edges` for row-sharded rasters: the plane holds H rows, rows
    # [y0, y1) are produced (compact output); edges bit 0 / 1 = row 0 / row H - 1 is a true image edge (include/rsseg.h).
    @staticmethod
    def _rows(H, rows):
        return (0, H) if rows is None else (int(rows[0]), int(rows[1]))

    def resize_bilinear_multi(self, srcs: Sequence, sh_local: int, sw: int, src_row0: int, sh: int, dh_local: int, dw: int, dst_row0: int, dh: int):
        """cv2.resize(INTER_LINEAR) of up to 8 maps of one shape in one launch (rows form; full maps: src_row0 = dst_row0 = 0)."""
        torch = _torch()
        dsts = [self.empty(dh_local * dw, torch.float32) for _ in srcs]
        self._chk(self.lib.rsseg_resize_bilinear_rows_multi_f32(self.h, self._pp(srcs), len(srcs), sh_local, sw, src_row0, sh, self._pp(dsts), dh_local,
                                                                dw, dst_row0, dh))
        self._tag_minmax(dsts)
        return dsts

    def box_mean(self, plane, H: int, W: int, k: int, border: int, square: bool = False, rows=None, edges: int = 3):
        return self.box_mean_multi([plane], H, W, k, border, square, rows, edges)[0]

    def box_mean_multi(self, planes: Sequence, H: int, W: int, k: int, border: int, square: bool = False, rows=None, edges: int = 3):
        """k x k box mean of up to 8 planes of equal shape in one launch (add_spatial_context, indices.py:760-776)."""
        torch = _torch()
        y0, y1 = self._rows(H, rows)
        outs = []
        for g in range(0, len(planes), 8):
            grp = list(planes[g:g + 8])
            o = [self.empty((y1 - y0) * W, torch.float32) for _ in grp]
            self._chk(self.lib.rsseg_box_mean_rows_f32(self.h, self._pp(grp), len(grp), H, W, y0, y1, edges, k, border, int(square), self._pp(o)))
            outs += o
        return outs

    def local_std(self, plane, H: int, W: int, k: int, rows=None, edges: int = 3, variance: bool = False):
        torch = _torch()
        y0, y1 = self._rows(H, rows)
        out = self.empty((y1 - y0) * W, torch.float32)
        self._chk(self.lib.rsseg_local_std_rows_f32(self.h, C.c_void_p(plane.data_ptr()), H, W, y0, y1, edges, k, int(variance),
                                                    C.c_void_p(out.data_ptr())))
        return out

    def local_var(self, plane, H: int, W: int, k: int, rows=None, edges: int = 3):
        return self.local_std(plane, H, W, k, rows, edges, variance=True)

    def morph(self, q, H: int, W: int, k: int, op: int, rows=None, edges: int = 3):
        """op: L.MORPH_ERODE / DILATE / OPEN / CLOSE / GRADIENT on a uint8 plane; uint8 result."""
        torch = _torch()
        y0, y1 = self._rows(H, rows)
        out = self.empty((y1 - y0) * W, torch.uint8)
        self._chk(self.lib.rsseg_morph_rows_u8(self.h, C.c_void_p(q.data_ptr()), H, W, y0, y1, edges, k, op, C.c_void_p(out.data_ptr())))
        return out

    def morph_gradient(self, q, H: int, W: int, k: int, rows=None, edges: int = 3):
        return self.morph(q, H, W, k, L.MORPH_GRADIENT, rows, edges)

    def laplacian_norm(self, q, H: int, W: int, rows=None, edges: int = 3):
        torch = _torch()
        y0, y1 = self._rows(H, rows)
        out = self.empty((y1 - y0) * W, torch.float32)
        self._chk(self.lib.rsseg_laplacian_norm_rows_u8(self.h, C.c_void_p(q.data_ptr()), H, W, y0, y1, edges, C.c_void_p(out.data_ptr())))
        return out

    def sobel_mag(self, q, H: int, W: int, rows=None, edges: int = 3):
        torch = _torch()
        y0, y1 = self._rows(H, rows)
        out = self.empty((y1 - y0) * W, torch.float32)
        self._chk(self.lib.rsseg_sobel_mag_rows_u8(self.h, C.c_void_p(q.data_ptr()), H, W, y0, y1, edges, C.c_void_p(out.data_ptr())))
        return out

    # ---- K17: correlation with a bank of float32 kernels -------------------------------------------
    @staticmethod
    def _taps(taps):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        if t.ndim == 2:
            t = t[None]
        if t.ndim != 3 or t.shape[1] != t.shape[2]:
            raise ValueError("taps: (nf, ksize, ksize) float32")
        return t

    def correlate_u8(self, q, H: int, W: int, taps, minmax: bool = False):
        """cv2.filter2D(u8, CV_32F, k)'s direct path for every k of taps[nf, ksize, ksize]: nf raw float32 planes (views of one
        buffer), and with minmax=True the (nf, 2) float32 array of their {min, max} beside them."""
        torch = _torch()
        t = self._taps(taps)
        nf, ksize = t.shape[0], t.shape[1]
        out = self.empty(max(nf, 1) * H * W, torch.float32)
        mm = np.zeros((max(nf, 1), 2), np.float32)
        self._chk(self.lib.rsseg_correlate_u8_f32(self.h, C.c_void_p(q.data_ptr()), H, W, t.ctypes.data_as(C.POINTER(C.c_float)), ksize, nf,
                                                  C.c_void_p(out.data_ptr()), mm.ctypes.data_as(C.POINTER(C.c_float)) if minmax else None))
        planes = [out[f * H * W:(f + 1) * H * W] for f in range(nf)]
        return (planes, mm) if minmax else planes

    def filter_bank_norm(self, q, H: int, W: int, taps):
        """correlate_u8, then every plane (r - min) / (max - min + 1e-10) in float32, in place."""
        torch = _torch()
        t = self._taps(taps)
        nf, ksize = t.shape[0], t.shape[1]
        out = self.empty(max(nf, 1) * H * W, torch.float32)
        self._chk(self.lib.rsseg_filter_bank_norm_u8(self.h, C.c_void_p(q.data_ptr()), H, W, t.ctypes.data_as(C.POINTER(C.c_float)), ksize, nf,
                                                     C.c_void_p(out.data_ptr())))
        return [out[f * H * W:(f + 1) * H * W] for f in range(nf)]

    # ---- K13: LBP, rank entropy, fixed-point Gaussian ---------------------------------------------
    def lbp_uniform(self, q, H: int, W: int, n_points: int = 24, radius: float = 3):
        torch = _torch()
        out = self.empty(H * W, torch.uint8)
        self._chk(self.lib.rsseg_lbp_uniform_u8(self.h, C.c_void_p(q.data_ptr()), H, W, n_points, C.c_double(radius), C.c_void_p(out.data_ptr())))
        return out

    def rank_entropy(self, q, H: int, W: int, radius: int):
        torch = _torch()
        out = self.empty(H * W, torch.float64)
        self._chk(self.lib.rsseg_rank_entropy_u8(self.h, C.c_void_p(q.data_ptr()), H, W, radius, C.c_void_p(out.data_ptr())))
        return out

    def gaussian_blur_u8(self, q, H: int, W: int, ksize: int):
        torch = _torch()
        out = self.empty(H * W, torch.uint8)
        self._chk(self.lib.rsseg_gaussian_blur_u8(self.h, C.c_void_p(q.data_ptr()), H, W, ksize, C.c_void_p(out.data_ptr())))
        return out

    # ---- K12: rule-based classification -------------------------------------------------------
    def threshold_band(self, plane, lo: float = float("-inf"), hi: float = float("inf"), nan_as_zero: bool = True):
        """uint8 mask: 1 where lo < x < hi.  nan_as_zero: NaN counts as 0 (threshold_segmentation, extract.py:354-356);
        False: a NaN pixel is outside every interval (the plain comparisons of extract_bareland_by_rule, extract.py:486-497)."""
        torch = _torch()
        out = self.empty(plane.numel(), torch.uint8)
        if plane.dtype == torch.float64:
            self._chk(self.lib.rsseg_band_interval_f64(self.h, C.c_void_p(plane.data_ptr()), plane.numel(), C.c_double(lo), C.c_double(hi),
                                                       int(nan_as_zero), C.c_void_p(out.data_ptr())))
            return out
        self._chk(self.lib.rsseg_band_interval_f32(self.h, C.c_void_p(plane.data_ptr()), plane.numel(), C.c_float(lo), C.c_float(hi),
                                                   int(nan_as_zero), C.c_void_p(out.data_ptr())))
        return out

    def otsu_mask(self, plane, above: bool = True):
        """threshold_segmentation(..., otsu=True) (extract.py:358-371) of a float32 / float64 plane -> (uint8 mask, level or -1
        when the plane has no contrast, min, max)."""
        torch = _torch()
        if plane.dtype not in (torch.float32, torch.float64):
            raise ValueError("otsu_mask: float32 or float64 plane expected")
        out = self.empty(plane.numel(), torch.uint8)
        level, mn, mx = C.c_int(0), C.c_double(0), C.c_double(0)
        self._chk(self.lib.rsseg_otsu_mask(self.h, C.c_void_p(plane.data_ptr()), L.F32 if plane.dtype == torch.float32 else L.F64,
                                           plane.numel(), int(bool(above)), C.c_void_p(out.data_ptr()), C.byref(level), C.byref(mn), C.byref(mx)))
        return out, level.value, mn.value, mx.value

    def fill_holes(self, mask, H: int, W: int):
        """scipy.ndimage.binary_fill_holes of a 0 / 1 uint8 plane (extract.py:314-316)."""
        torch = _torch()
        out = self.empty(H * W, torch.uint8)
        self._chk(self.lib.rsseg_fill_holes_u8(self.h, C.c_void_p(mask.data_ptr()), H, W, C.c_void_p(out.data_ptr())))
        return out

    def mask_op(self, a, b, op: int):
        torch = _torch()
        out = self.empty(a.numel(), torch.uint8)
        self._chk(self.lib.rsseg_mask_op_u8(self.h, C.c_void_p(a.data_ptr()), None if b is None else C.c_void_p(b.data_ptr()), a.numel(), op,
                                            C.c_void_p(out.data_ptr())))
        return out

    def mask_paint(self, final_map, mask, value: int, only_unset: bool = False):
        self._chk(self.lib.rsseg_mask_paint_u8(self.h, C.c_void_p(final_map.data_ptr()), C.c_void_p(mask.data_ptr()), final_map.numel(), value,
                                               int(only_unset)))
        return final_map

    def morph_ellipse(self, q, H: int, W: int, k: int, op: int):
        torch = _torch()
        out = self.empty(H * W, torch.uint8)
        self._chk(self.lib.rsseg_morph_ellipse_u8(self.h, C.c_void_p(q.data_ptr()), H, W, k, op, C.c_void_p(out.data_ptr())))
        return out

    def remove_small_components(self, mask, H: int, W: int, min_area: int):
        torch = _torch()
        out = self.empty(H * W, torch.uint8)
        self._chk(self.lib.rsseg_remove_small_components_u8(self.h, C.c_void_p(mask.data_ptr()), H, W, int(min_area), C.c_void_p(out.data_ptr())))
        return out

    # ---- K20: class-map clean-up (rsseg/postclass.py) --------------------------------------------
    def hist_u8(self, q) -> np.ndarray:
        """How often every byte value occurs in a uint8 device plane: int64[256]."""
        counts = np.zeros(256, np.int64)
        self._chk(self.lib.rsseg_hist_u8(self.h, C.c_void_p(q.data_ptr()), q.numel(), counts.ctypes.data_as(C.POINTER(C.c_int64))))
        return counts

    def replace_u8(self, q, old: int, new: int) -> int:
        """q[q == old] = new in place on a uint8 device plane; how many pixels that was."""
        n = C.c_int64(0)
        self._chk(self.lib.rsseg_replace_u8(self.h, C.c_void_p(q.data_ptr()), q.numel(), int(old), int(new), C.byref(n)))
        return n.value

    def majority_u8(self, q, H: int, W: int, k: int, ignore: int = -1, fill: int = -1, fill_only: bool = False, rows=None, image_rows=None,
                    group_mask: int = 0, out=None):
        """k x k majority filter of a uint8 class map (include/rsseg.h, rsseg_majority_u8): (out, n_changed, n_unfilled).
        rows=(y0, y1): the plane holds H rows and rows [y0, y1) are produced (compact output); image_rows=(img_y0, img_H):
        the plane is rows [img_y0, img_y0 + H) of an image img_H rows tall, against whose edges the window is clipped
        (default: the plane is the image).  group_mask: bit g when a label in 8g .. 8g + 7 may occur; 0 = found in the call."""
        torch = _torch()
        y0, y1 = self._rows(H, rows)
        img_y0, img_h = (0, H) if image_rows is None else (int(image_rows[0]), int(image_rows[1]))
        if out is None:   # `out`: a uint8 plane of (y1 - y0) * W pixels to write instead (repeated passes ping-pong two buffers)
            out = self.empty(max((y1 - y0) * W, 1), torch.uint8)[:max(y1 - y0, 0) * W]   # an empty stripe still hands the library a pointer
        nc, nu = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.rsseg_majority_u8(self.h, C.c_void_p(q.data_ptr()), H, W, y0, y1, img_y0, img_h, int(k), int(ignore), int(fill),
                                             int(bool(fill_only)), int(group_mask), C.c_void_p(out.data_ptr()), C.byref(nc), C.byref(nu)))
        return out, nc.value, nu.value

    def sieve_u8(self, q, H: int, W: int, min_area: int, connectivity: int = 8, ignore: int = 0, removed_value: int = 0):
        """Multi-class sieve (rsseg_sieve_u8): same-label components of fewer than min_area pixels become removed_value;
        (out, n_removed).  Whole raster on one GPU."""
        torch = _torch()
        out = self.empty(H * W, torch.uint8)
        nr = C.c_int64(0)
        self._chk(self.lib.rsseg_sieve_u8(self.h, C.c_void_p(q.data_ptr()), H, W, int(min_area), int(connectivity), int(ignore), int(removed_value),
                                          C.c_void_p(out.data_ptr()), C.byref(nr)))
        return out, nr.value

    # ---- K23: superpixels and per-segment reductions (rsseg/segment.py) ---------------------------
    def slic_tile(self) -> Tuple[int, int]:
        """(columns, rows) of the assignment kernel's tile."""
        tw, th = C.c_int(0), C.c_int(0)
        self.lib.rsseg_slic_tile(C.byref(tw), C.byref(th))
        return tw.value, th.value

    def slic_u8(self, planes: Sequence, H: int, W: int, step: int, weight: float, max_iter: int = 10, min_area: int = 0, mask=None):
        """SLIC superpixels of uint8 device planes (include/rsseg.h, rsseg_slic_u8): (labels int32 of H * W with 0 = masked and
        1 ... n_segments, n_segments, n_iter, n_regrown).  mask: None or a uint8 plane, 0 = not valid."""
        torch = _torch()
        labels = self.empty(H * W, torch.int32)
        ns, ni, nr = C.c_int64(0), C.c_int(0), C.c_int64(0)
        self._chk(self.lib.rsseg_slic_u8(self.h, self._pp(planes), len(planes), int(H), int(W), None if mask is None else C.c_void_p(mask.data_ptr()),
                                         int(step), C.c_double(weight), int(max_iter), int(min_area), C.c_void_p(labels.data_ptr()), C.byref(ns),
                                         C.byref(ni), C.byref(nr)))
        return labels, ns.value, ni.value, nr.value

    def segment_sums(self, seg, H: int, W: int, n_segments: int, planes: Sequence = (), mask=None):
        """int64 device table [(n_segments + 1), 3 + P] of rsseg_segment_sums: area, sum y, sum x and the sum of every plane per
        segment (uint8 planes as integers, float32 planes in units of 2^-40).  At most 16 planes of one dtype per call."""
        torch = _torch()
        P = len(planes)
        u8 = [self._is_u8(p) for p in planes]
        if any(u8) and not all(u8):
            raise ValueError("segment_sums: uint8 and float32 planes cannot be mixed in one call")
        if P and not all(u8) and any(p.dtype != torch.float32 for p in planes):
            raise ValueError("segment_sums: planes must be uint8 or float32")
        out = self.empty((int(n_segments) + 1) * (3 + P), torch.int64)
        self._chk(self.lib.rsseg_segment_sums(self.h, C.c_void_p(seg.data_ptr()), int(H), int(W), int(n_segments), self._pp(planes) if P else None, P,
                                              L.U8 if (P == 0 or all(u8)) else L.F32, None if mask is None else C.c_void_p(mask.data_ptr()),
                                              C.c_void_p(out.data_ptr())))
        return out.reshape(int(n_segments) + 1, 3 + P)

    def segment_majority_u8(self, seg, n_segments: int, class_map, ignore: int = -1, fill: int = 0):
        """uint8 device table [n_segments + 1] of rsseg_segment_majority_u8: every segment's most frequent label of class_map
        (ties: the smallest; `ignore` never votes; no voter, and entry 0: `fill`)."""
        torch = _torch()
        table = self.empty(int(n_segments) + 1, torch.uint8)
        self._chk(self.lib.rsseg_segment_majority_u8(self.h, C.c_void_p(seg.data_ptr()), seg.numel(), int(n_segments), C.c_void_p(class_map.data_ptr()),
                                                     int(ignore), int(fill), C.c_void_p(table.data_ptr())))
        return table

    def segment_paint(self, seg, n_segments: int, table):
        """out[i] = table[seg[i]] for a uint8, float32 or int32 device table of n_segments + 1 entries."""
        if table.numel() != int(n_segments) + 1 or table.element_size() not in (1, 4):
            raise ValueError(f"segment_paint: the table has {table.numel()} entries of {table.element_size()} bytes, "
                             f"{int(n_segments) + 1} of 1 or 4 bytes are needed")
        out = self.empty(seg.numel(), table.dtype)
        self._chk(self.lib.rsseg_segment_paint(self.h, C.c_void_p(seg.data_ptr()), seg.numel(), int(n_segments), C.c_void_p(table.data_ptr()),
                                               table.element_size(), C.c_void_p(out.data_ptr())))
        return out

    # ---- K25: the object table (rsseg/objects.py) -------------------------------------------------
    def segment_features_plan(self, P: int = 0) -> Tuple[int, int, int]:
        """(tile columns, tile rows, rows of the per-tile LDS table) of rsseg_segment_features."""
        tw, th, ns = C.c_int(0), C.c_int(0), C.c_int(0)
        self.lib.rsseg_segment_features_plan(int(P), C.byref(tw), C.byref(th), C.byref(ns))
        return tw.value, th.value, ns.value

    def segment_features(self, seg, H: int, W: int, n_segments: int, planes: Sequence = (), mask=None, geometry: bool = True):
        """int64 device table [(n_segments + 1), 11 + 4 P] of rsseg_segment_features: n, the coordinate moments, the bounding
        box and the perimeter (geometry=False leaves columns 1 ... 10 at their empty values), then per plane sum, sum of squares,
        min and max (uint8 planes as integers, float32 planes in units of 2^-40 and 2^-24).  At most 16 planes of one dtype."""
        torch = _torch()
        P = len(planes)
        u8 = [self._is_u8(p) for p in planes]
        if any(u8) and not all(u8):
            raise ValueError("segment_features: uint8 and float32 planes cannot be mixed in one call")
        if P and not all(u8) and any(p.dtype != torch.float32 for p in planes):
            raise ValueError("segment_features: planes must be uint8 or float32")
        cols = 11 + 4 * P
        out = self.empty((int(n_segments) + 1) * cols, torch.int64)
        self._chk(self.lib.rsseg_segment_features(self.h, C.c_void_p(seg.data_ptr()), int(H), int(W), int(n_segments), self._pp(planes) if P else None, P,
                                                  L.U8 if (P == 0 or all(u8)) else L.F32, None if mask is None else C.c_void_p(mask.data_ptr()),
                                                  L.OBJ_GEOMETRY if geometry else 0, C.c_void_p(out.data_ptr())))
        return out.reshape(int(n_segments) + 1, cols)

    # ---- K27: the region adjacency graph (rsseg/regions.py) ----------------------------------------
    def segment_adjacency_plan(self, P: int = 0) -> Tuple[int, int, int]:
        """(tile columns, tile rows, rows of the per-tile LDS table) of rsseg_segment_adjacency."""
        tw, th, ns = C.c_int(0), C.c_int(0), C.c_int(0)
        self.lib.rsseg_segment_adjacency_plan(int(P), C.byref(tw), C.byref(th), C.byref(ns))
        return tw.value, th.value, ns.value

    def segment_adjacency(self, seg, H: int, W: int, n_segments: int, planes: Sequence = (), mask=None, max_edges: Optional[int] = None):
        """int64 device table [E, 3 + P] of rsseg_segment_adjacency, sorted ascending by (a, b): per pair of adjacent segments
        a < b the length of their border and, per uint8 plane, the summed absolute step across it.  max_edges: the rows the
        call may fill (RssegUnsupported when the raster holds more pairs).  None: 4 n_segments + 64 rows, and on that refusal
        once more with min(2 H W - H - W, n (n - 1) / 2), which no raster exceeds; MemoryError when that cannot be allocated."""
        torch = _torch()
        P = len(planes)
        if any(not self._is_u8(p) for p in planes):
            raise ValueError("segment_adjacency: planes must be uint8")
        H, W, n = int(H), int(W), int(n_segments)
        if max_edges is None:
            tries = [4 * n + 64, max(0, min(2 * H * W - H - W, n * (n - 1) // 2))]
        else:
            tries = [int(max_edges)]
        cols = 3 + P
        for i, cap in enumerate(tries):
            try:
                out = torch.empty(max(cap, 1) * cols, dtype=torch.int64, device=self.device)
            except torch.cuda.OutOfMemoryError as e:
                raise MemoryError(f"segment_adjacency: {cap} rows of {cols} int64 could not be allocated") from e
            ne = C.c_int64(0)
            try:
                self._chk(self.lib.rsseg_segment_adjacency(self.h, C.c_void_p(seg.data_ptr()), H, W, n, None if mask is None else C.c_void_p(mask.data_ptr()),
                                                           self._pp(planes) if P else None, P, cap, C.c_void_p(out.data_ptr()), C.byref(ne)))
            except RssegUnsupported:
                if i + 1 < len(tries) and 0 <= P <= 16 and tries[i + 1] > cap:
                    continue
                raise
            rows = out[:ne.value * cols].reshape(ne.value, cols)
            order = torch.argsort((rows[:, 0] << 32) | rows[:, 1])
            return rows[order].contiguous()

    # ---- K9/K10 --------------------------------------------------------------------------------
    def kmeans_fit_predict(self, planes: Sequence, n_clusters: int, seed: int = 42, max_iter: int = 300, tol: float = 1e-4):
        torch = _torch()
        F, n = len(planes), planes[0].numel()
        dt = planes[0].dtype
        if any(p.dtype != dt for p in planes) or dt not in (torch.float32, torch.float64):
            raise ValueError("kmeans planes must all be float32 or all float64")
        labels = self.empty(max(n, 1), torch.int32)
        centers = np.zeros((n_clusters, F), np.float64)
        info = L.KMeansInfo()
        tags = [getattr(p, "_rsseg_minmax", None) for p in planes]
        if dt == torch.float32 and n > 0 and all(t is not None for t in tags):
            lmin = (C.c_double * F)(*[t[0] for t in tags])
            lmax = (C.c_double * F)(*[t[1] for t in tags])
            self._chk(self.lib.rsseg_kmeans_fit_predict_mm(self.h, self._pp(planes), F, L.F32, n, n_clusters, seed, max_iter, tol,
                                                           C.c_void_p(labels.data_ptr()), centers.ctypes.data_as(C.POINTER(C.c_double)),
                                                           C.byref(info), lmin, lmax))
        else:
            self._chk(self.lib.rsseg_kmeans_fit_predict(self.h, self._pp(planes), F, L.F32 if dt == torch.float32 else L.F64, n,
                                                        n_clusters, seed, max_iter, tol, C.c_void_p(labels.data_ptr()),
                                                        centers.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info)))
        meta = dict(n_iter=info.n_iter, tol=info.tol, relocated=info.relocated,
                    scale=np.array(info.scale[:F]), min=np.array(info.min[:F]), mean=np.array(info.mean[:F]),
                    init_indices=np.array(info.init_indices[:n_clusters]), ms_init=info.ms_init, ms_lloyd=info.ms_lloyd,
                    centers=centers)
        return labels[:n], meta

    # ---- K18 -----------------------------------------------------------------------------------
    def kmeans_predict(self, planes: Sequence, centers, scale, min_, want_distance: bool = False, want_summary: bool = False):
        """A fitted model (cluster_centers_, MinMaxScaler scale_ / min_) applied to planes: (labels int32, distance in the planes'
        dtype or None, summary dict or None).  The summary is this context's own (nothing is reduced across ranks)."""
        torch = _torch()
        F, n = len(planes), planes[0].numel() if len(planes) else 0
        if F == 0:
            raise ValueError("kmeans: no feature planes")
        dt = planes[0].dtype
        if any(p.dtype != dt for p in planes) or dt not in (torch.float32, torch.float64):
            raise ValueError("kmeans planes must all be float32 or all float64")
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        scale = np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
        min_ = np.ascontiguousarray(min_, dtype=np.float64).reshape(-1)
        if centers.ndim != 2 or centers.shape[1] != F or scale.size != F or min_.size != F:
            raise ValueError(f"kmeans_predict: the model has {centers.shape[-1] if centers.ndim else 0} features "
                             f"(scale {scale.size}, min_ {min_.size}), the call {F} planes")
        k = centers.shape[0]
        labels = self.empty(max(n, 1), torch.int32)
        dist = self.empty(max(n, 1), dt) if want_distance else None
        info = L.KMeansApplyInfo() if want_summary else None
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.rsseg_kmeans_predict(self.h, self._pp(planes), F, L.F32 if dt == torch.float32 else L.F64, n, k,
                                                centers.ctypes.data_as(dp), scale.ctypes.data_as(dp), min_.ctypes.data_as(dp),
                                                C.c_void_p(labels.data_ptr()), C.c_void_p(dist.data_ptr()) if want_distance else None,
                                                C.byref(info) if want_summary else None))
        summary = None
        if want_summary:
            summary = dict(counts=np.array(info.counts[:k], dtype=np.int64), inertia=float(info.inertia), overflow=bool(info.overflow),
                           ms=info.ms)
        return labels[:n], (dist[:n] if want_distance else None), summary

    # ---- K19: valid masks and order-preserving compaction --------------------------------------
    def valid_mask(self, planes: Sequence, nan: bool = True, inf: bool = False, nodata=None, and_mask=None):
        """(uint8 mask, n_valid): a pixel is valid iff no plane holds a NaN (`nan`), +-inf (`inf`) or `nodata` (cast to the
        planes' dtype) there and, when given, and_mask is non-zero there.  planes: flat float32, float64 or uint8 device
        tensors of one dtype and length."""
        torch = _torch()
        if not len(planes):
            raise ValueError("valid_mask: no planes")
        dt, n = planes[0].dtype, planes[0].numel()
        codes = {torch.float32: L.F32, torch.float64: L.F64, torch.uint8: L.U8}
        if dt not in codes or any(p.dtype != dt or p.numel() != n for p in planes):
            raise ValueError("valid_mask: planes must be float32, float64 or uint8, all of one dtype and length")
        if and_mask is not None and (and_mask.dtype != torch.uint8 or and_mask.numel() != n):
            raise ValueError("valid_mask: and_mask must be a uint8 plane of the planes' length")
        flags = (L.VALID_NAN if nan else 0) | (L.VALID_INF if inf else 0) | (L.VALID_VALUE if nodata is not None else 0)
        mask = self.empty(max(n, 1), torch.uint8)
        nv = C.c_int64(0)
        self._chk(self.lib.rsseg_valid_mask(self.h, self._pp(planes), len(planes), codes[dt], n, flags,
                                            C.c_double(0.0 if nodata is None else float(nodata)),
                                            None if and_mask is None else C.c_void_p(and_mask.data_ptr()), C.c_void_p(mask.data_ptr()),
                                            C.byref(nv)))
        return mask[:n], int(nv.value)

    def compact_plan(self, mask) -> "CompactPlan":
        """The plan compact() and expand() share for one mask (a flat uint8 device tensor, non-zero = valid): the tile offsets
        live in a tensor of the plan's own, not in the context's workspace, so a classifier call may run in between."""
        torch = _torch()
        if mask.dtype != torch.uint8:
            raise ValueError("compact_plan: the mask must be a uint8 plane")
        n = mask.numel()
        tile = self.lib.rsseg_compact_tile()
        off = self.empty((n + tile - 1) // tile + 1, torch.int64)
        nv = C.c_int64(0)
        self._chk(self.lib.rsseg_compact_plan(self.h, C.c_void_p(mask.data_ptr()) if n else None, n, C.c_void_p(off.data_ptr()), C.byref(nv)))
        return CompactPlan(mask, off, n, int(nv.value))

    def compact(self, plan: "CompactPlan", planes: Sequence) -> List:
        """planes[p][mask != 0] for every plane, in raster order: a list of new tensors of plan.n_valid elements.  Planes of one
        element size (1, 4 or 8 bytes) share a launch."""
        outs = [None] * len(planes)
        by_size = {}
        for i, p in enumerate(planes):
            if p.numel() != plan.n:
                raise ValueError(f"compact: plane {i} has {p.numel()} elements, the mask {plan.n}")
            by_size.setdefault(p.element_size(), []).append(i)
        for eb, idx in by_size.items():
            if eb not in (1, 4, 8):
                raise ValueError(f"compact: elements of {eb} bytes (1, 4 or 8 are taken)")
            full = [self.empty(max(plan.n_valid, 1), planes[i].dtype) for i in idx]
            self._chk(self.lib.rsseg_compact_planes(self.h, C.c_void_p(plan.mask.data_ptr()) if plan.n else None,
                                                    C.c_void_p(plan.tile_off.data_ptr()), plan.n, self._pp([planes[i] for i in idx]), len(idx), eb,
                                                    self._pp(full)))
            for i, t in zip(idx, full):
                outs[i] = t[:plan.n_valid]
        return outs

    def expand(self, plan: "CompactPlan", plane, fill):
        """A tensor of plan.n elements: plane[rank(i)] where the mask is set, `fill` (cast to the plane's dtype) elsewhere."""
        torch = _torch()
        if plane.numel() != plan.n_valid:
            raise ValueError(f"expand: the plane has {plane.numel()} elements, the mask {plan.n_valid} valid pixels")
        eb = plane.element_size()
        if eb not in (1, 4, 8):
            raise ValueError(f"expand: elements of {eb} bytes (1, 4 or 8 are taken)")
        fb = np.array(fill, dtype=torch.empty(0, dtype=plane.dtype).numpy().dtype).tobytes()
        out = self.empty(max(plan.n, 1), plane.dtype)
        self._chk(self.lib.rsseg_expand_plane(self.h, C.c_void_p(plan.mask.data_ptr()) if plan.n else None, C.c_void_p(plan.tile_off.data_ptr()),
                                              plan.n, C.c_void_p(plane.data_ptr()) if plan.n_valid else None, eb, fb, C.c_void_p(out.data_ptr())))
        return out[:plan.n]

    # ---- K22: Gaussian maximum-likelihood / Mahalanobis / minimum-distance classification ---------
    def gauss_classify(self, planes: Sequence, mean, whiten, offset, class_values, max_dist2=float("inf"), want_dist2: bool = False,
                       want_margin: bool = False):
        """rsseg_gauss_classify (include/rsseg.h) on flat float32 / float64 device planes: (labels uint8, dist2 float32 or None,
        margin float32 or None).  mean (k, F), whiten (k, F (F + 1) / 2) the packed rows of the lower-triangular whitening
        matrices, offset (k,), class_values (k,) distinct in 1..255; max_dist2=inf: no threshold."""
        torch = _torch()
        F = len(planes)
        if F == 0:
            raise ValueError("gauss_classify: no feature planes")
        dt, n = planes[0].dtype, planes[0].numel()
        if any(p.dtype != dt or p.numel() != n for p in planes) or dt not in (torch.float32, torch.float64):
            raise ValueError("gauss_classify: planes must all be float32 or all float64, of one length")
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        offset = np.ascontiguousarray(offset, dtype=np.float64).reshape(-1)
        k = offset.size
        whiten = np.ascontiguousarray(whiten, dtype=np.float64).reshape(k, -1) if k else np.zeros((0, 0))
        cv = np.asarray(class_values).reshape(-1)
        if mean.ndim != 2 or mean.shape != (k, F) or whiten.shape != (k, F * (F + 1) // 2) or cv.size != k:
            raise ValueError(f"gauss_classify: the model's shapes (mean {mean.shape}, whiten {whiten.shape}, offset {offset.shape}, "
                             f"class_values {cv.shape}) do not describe k classes over the call's {F} planes")
        if np.any(cv != cv.astype(np.uint8)):
            raise ValueError("gauss_classify: class_values must be integers in 1..255")
        cv = np.ascontiguousarray(cv, dtype=np.uint8)
        labels = self.empty(max(n, 1), torch.uint8)
        dist2 = self.empty(max(n, 1), torch.float32) if want_dist2 else None
        margin = self.empty(max(n, 1), torch.float32) if want_margin else None
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.rsseg_gauss_classify(self.h, self._pp(planes), F, L.F32 if dt == torch.float32 else L.F64, n, k,
                                                mean.ctypes.data_as(dp), whiten.ctypes.data_as(dp), offset.ctypes.data_as(dp),
                                                cv.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_double(float(max_dist2)),
                                                C.c_void_p(labels.data_ptr()), C.c_void_p(dist2.data_ptr()) if want_dist2 else None,
                                                C.c_void_p(margin.data_ptr()) if want_margin else None))
        return labels[:n], (dist2[:n] if want_dist2 else None), (margin[:n] if want_margin else None)

    # ---- K28: support vector machine classification (rsseg/svm.py) ---------------------------------
    SVM_KERNELS = {"rbf": 0, "poly": 1, "linear": 2}   # RSSEG_SVM_*

    def svm_classify(self, planes: Sequence, offset, scale, sv, n_support, coef, bias, class_values, kernel="rbf", gamma: float = 1.0,
                     coef0: float = 0.0, degree: int = 3, w=None, want_margin: bool = False):
        """rsseg_svm_classify (include/rsseg.h) on flat float32 / float64 device planes: (labels uint8, margin float32 or None).
        offset, scale (F,); sv (S, F) in scaled units, grouped by class; n_support (k,); coef (k - 1, S); bias (k (k - 1) / 2,);
        class_values (k,) distinct in 1..255; kernel 'rbf' | 'poly' | 'linear' (or its RSSEG_SVM_* number); w (P, F) for 'linear'."""
        torch = _torch()
        F = len(planes)
        if F == 0:
            raise ValueError("svm_classify: no feature planes")
        dt, n = planes[0].dtype, planes[0].numel()
        if any(p.dtype != dt or p.numel() != n for p in planes) or dt not in (torch.float32, torch.float64):
            raise ValueError("svm_classify: planes must all be float32 or all float64, of one length")
        if isinstance(kernel, str):
            if kernel not in self.SVM_KERNELS:
                raise ValueError(f"svm_classify: kernel {kernel!r}, must be one of {tuple(self.SVM_KERNELS)}")
            kernel = self.SVM_KERNELS[kernel]
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)   # noqa: E731
        offset, scale, bias = f64(offset).reshape(-1), f64(scale).reshape(-1), f64(bias).reshape(-1)
        sv, coef = f64(sv), f64(coef)
        ns = np.asarray(n_support).reshape(-1)
        cv = np.asarray(class_values).reshape(-1)
        k = ns.size
        S = sv.shape[0] if sv.ndim == 2 else -1
        P = k * (k - 1) // 2
        if (offset.size != F or scale.size != F or sv.ndim != 2 or sv.shape[1] != F or coef.ndim != 2 or coef.shape != (k - 1, S) or bias.size != P
                or cv.size != k):
            raise ValueError(f"svm_classify: the model's shapes (offset {offset.shape}, scale {scale.shape}, sv {sv.shape}, n_support {ns.shape}, "
                             f"coef {coef.shape}, bias {bias.shape}, class_values {cv.shape}) do not describe k classes over the call's {F} planes")
        if np.any(ns != ns.astype(np.int32)):
            raise ValueError("svm_classify: n_support must be integers")
        if np.any(cv != cv.astype(np.uint8)):
            raise ValueError("svm_classify: class_values must be integers in 1..255")
        ns, cv = np.ascontiguousarray(ns, dtype=np.int32), np.ascontiguousarray(cv, dtype=np.uint8)
        if w is not None:
            w = f64(w)
            if w.shape != (P, F):
                raise ValueError(f"svm_classify: w {w.shape}, the folded weights of {k} classes over {F} planes are {(P, F)}")
        labels = self.empty(max(n, 1), torch.uint8)
        margin = self.empty(max(n, 1), torch.float32) if want_margin else None
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.rsseg_svm_classify(self.h, self._pp(planes), F, L.F32 if dt == torch.float32 else L.F64, n, k, S,
                                              offset.ctypes.data_as(dp), scale.ctypes.data_as(dp), sv.ctypes.data_as(dp),
                                              ns.ctypes.data_as(C.POINTER(C.c_int)), coef.ctypes.data_as(dp), bias.ctypes.data_as(dp),
                                              cv.ctypes.data_as(C.POINTER(C.c_uint8)), int(kernel), C.c_double(float(gamma)), C.c_double(float(coef0)),
                                              int(degree), None if w is None else w.ctypes.data_as(dp), C.c_void_p(labels.data_ptr()),
                                              C.c_void_p(margin.data_ptr()) if want_margin else None))
        return labels[:n], (margin[:n] if want_margin else None)

    # ---- K30: neural-network classification (rsseg/mlp.py) ------------------------------------------
    MLP_ACTIVATIONS = {"relu": 0, "identity": 1, "logistic": 2, "tanh": 3}   # RSSEG_MLP_*

    def mlp_plan(self, widths, k: int) -> Tuple[bool, int]:
        """(fits, tile_pixels) of rsseg_mlp_classify for layers of these widths (F, the hidden widths, the output units) and k
        classes: whether the staged model fits LDS, and the pixels a workgroup takes at a time (0 when it does not)."""
        w = np.ascontiguousarray(widths, dtype=np.int32).reshape(-1)
        fits, tile = C.c_int(0), C.c_int(0)
        self.lib.rsseg_mlp_plan(int(w[0]) if w.size else 0, int(w.size) - 1, w.ctypes.data_as(C.POINTER(C.c_int)), int(k), C.byref(fits), C.byref(tile))
        return bool(fits.value), tile.value

    def mlp_classify(self, planes: Sequence, widths, weights, biases, offset, scale, activation, class_values, want_margin: bool = False,
                     want_conf: bool = False, want_proba: bool = False):
        """rsseg_mlp_classify (include/rsseg.h) on flat float32 device planes: (labels uint8, margin, conf float32 (n,), proba
        float32 (k, n)), each of the last three None unless wanted.  widths: F, the hidden widths, the output units (1 for two
        classes); weights / biases: the layers' coefs_ / intercepts_ flattened and concatenated (float32); offset, scale (F,);
        activation 'relu' | 'identity' | 'logistic' | 'tanh' (or its RSSEG_MLP_* number); class_values (k,) distinct in 1..255."""
        torch = _torch()
        F = len(planes)
        if F == 0:
            raise ValueError("mlp_classify: no feature planes")
        n = planes[0].numel()
        if any(p.dtype != torch.float32 or p.numel() != n for p in planes):
            raise ValueError("mlp_classify: planes must all be float32, of one length")
        if isinstance(activation, str):
            if activation not in self.MLP_ACTIVATIONS:
                raise ValueError(f"mlp_classify: activation {activation!r}, must be one of {tuple(self.MLP_ACTIVATIONS)}")
            activation = self.MLP_ACTIVATIONS[activation]
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).reshape(-1)   # noqa: E731
        weights, biases, offset, scale = f32(weights), f32(biases), f32(offset), f32(scale)
        w = np.asarray(widths).reshape(-1)
        cv = np.asarray(class_values).reshape(-1)
        k = cv.size
        if w.size < 2 or np.any(w != w.astype(np.int32)):
            raise ValueError(f"mlp_classify: widths {w.tolist()} are not the integer widths of an input and at least one more layer")
        w = np.ascontiguousarray(w, dtype=np.int32)
        n_w, n_b = int((w[:-1].astype(np.int64) * w[1:]).sum()), int(w[1:].sum())
        if offset.size != F or scale.size != F or weights.size != n_w or biases.size != n_b or int(w[0]) != F:
            raise ValueError(f"mlp_classify: the model's shapes (widths {w.tolist()}, {weights.size} weights, {biases.size} biases, offset {offset.shape}, "
                             f"scale {scale.shape}) do not describe layers over the call's {F} planes")
        if np.any(cv != cv.astype(np.uint8)):
            raise ValueError("mlp_classify: class_values must be integers in 1..255")
        cv = np.ascontiguousarray(cv, dtype=np.uint8)
        labels = self.empty(max(n, 1), torch.uint8)
        margin = self.empty(max(n, 1), torch.float32) if want_margin else None
        conf = self.empty(max(n, 1), torch.float32) if want_conf else None
        proba = self.empty(max(n, 1) * max(k, 1), torch.float32) if want_proba else None
        fp = C.POINTER(C.c_float)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        self._chk(self.lib.rsseg_mlp_classify(self.h, self._pp(planes), F, n, int(w.size) - 1, w.ctypes.data_as(C.POINTER(C.c_int)),
                                              weights.ctypes.data_as(fp), biases.ctypes.data_as(fp), offset.ctypes.data_as(fp),
                                              scale.ctypes.data_as(fp), int(activation), k, cv.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              ptr(labels), ptr(margin), ptr(conf), ptr(proba)))
        return (labels[:n], margin[:n] if want_margin else None, conf[:n] if want_conf else None,
                proba[:k * n].reshape(k, n) if want_proba else None)

    # ---- K24: class signatures (rsseg/signatures.py) ----------------------------------------------
    def class_moments_plan(self, F: int, n_classes: int, u8: bool = False) -> Tuple[int, int]:
        """(path, tile_pixels) of rsseg_class_moments for F planes and n_classes labels: path 0 keeps the workgroup's table in
        LDS, 1 adds into the global table."""
        path, tile = C.c_int(0), C.c_int(0)
        self.lib.rsseg_class_moments_plan(int(F), int(n_classes), L.U8 if u8 else L.F32, C.byref(path), C.byref(tile))
        return path.value, tile.value

    def class_moments(self, planes: Sequence, labels, n_classes: int, plane_exp, Q: int, ignore: int = -1, mask=None):
        """rsseg_class_moments (include/rsseg.h) on flat float32 or uint8 device planes and a uint8 or int32 label plane:
        (int64 device table [n_classes, 1 + F + F (F + 1) / 2], n_left_out).  plane_exp: F ints for float32 planes, None for
        uint8 planes (whose Q is 0).  mask: None or a uint8 plane, 0 = not counted."""
        torch = _torch()
        F = len(planes)
        if F == 0:
            raise ValueError("class_moments: no feature planes")
        dt, n = planes[0].dtype, planes[0].numel()
        if any(p.dtype != dt or p.numel() != n for p in planes) or dt not in (torch.float32, torch.uint8):
            raise ValueError("class_moments: planes must all be float32 or all uint8, of one length")
        if labels.dtype not in (torch.uint8, torch.int32) or labels.numel() != n:
            raise ValueError("class_moments: labels must be a uint8 or int32 plane of the planes' length")
        if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != n):
            raise ValueError("class_moments: mask must be a uint8 plane of the planes' length")
        pe = None
        if plane_exp is not None:
            pe = np.ascontiguousarray(plane_exp, dtype=np.int32).reshape(-1)
            if pe.size != F:
                raise ValueError(f"class_moments: {pe.size} plane exponents for {F} planes")
        cols = 1 + F + F * (F + 1) // 2
        out = self.empty(max(int(n_classes), 1) * cols, torch.int64)
        left = C.c_int64(0)
        self._chk(self.lib.rsseg_class_moments(self.h, self._pp(planes), F, L.F32 if dt == torch.float32 else L.U8, n,
                                               C.c_void_p(labels.data_ptr()) if n else None, L.U8 if labels.dtype == torch.uint8 else L.I32,
                                               int(n_classes), int(ignore), None if mask is None else C.c_void_p(mask.data_ptr()),
                                               None if pe is None else pe.ctypes.data_as(C.POINTER(C.c_int)), int(Q), C.c_void_p(out.data_ptr()),
                                               C.byref(left)))
        return out.reshape(max(int(n_classes), 1), cols), left.value

    # ---- K26: ISODATA (rsseg/isodata.py) ------------------------------------------------------------
    def isodata_plan(self, F: int, k: int, u8: bool = False) -> Tuple[int, int]:
        """(path, tile_pixels) of rsseg_isodata_sweep for F planes and k centres: path 0 keeps the workgroup's table in LDS,
        1 adds into the global table."""
        path, tile = C.c_int(0), C.c_int(0)
        self.lib.rsseg_isodata_plan(int(F), int(k), L.U8 if u8 else L.F32, C.byref(path), C.byref(tile))
        return path.value, tile.value

    def isodata_sweep(self, planes: Sequence, labels, centers, weight, plane_exp, Q: int, mask=None, want_table: bool = True):
        """rsseg_isodata_sweep (include/rsseg.h) on flat float32 or uint8 device planes: every counted pixel is assigned to the
        nearest of the centres (k, F), in weighted units; `labels`, a uint8 device plane, is read and rewritten in place
        (255: not counted or left out).  -> (int64 device table [k, 1 + 2 F] or None when want_table is False, n_changed,
        n_left_out).  plane_exp: F ints for float32 planes, None for uint8 planes (whose Q is 0); mask: None or a uint8 plane,
        0 = not counted."""
        torch = _torch()
        F = len(planes)
        if F == 0:
            raise ValueError("isodata_sweep: no feature planes")
        dt, n = planes[0].dtype, planes[0].numel()
        if any(p.dtype != dt or p.numel() != n for p in planes) or dt not in (torch.float32, torch.uint8):
            raise ValueError("isodata_sweep: planes must all be float32 or all uint8, of one length")
        if labels.dtype != torch.uint8 or labels.numel() != n:
            raise ValueError("isodata_sweep: labels must be a uint8 plane of the planes' length")
        if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != n):
            raise ValueError("isodata_sweep: mask must be a uint8 plane of the planes' length")
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        weight = np.ascontiguousarray(weight, dtype=np.float64).reshape(-1)
        if centers.ndim != 2 or centers.shape[0] < 1 or centers.shape[1] != F or weight.size != F:
            raise ValueError(f"isodata_sweep: centers {centers.shape} and {weight.size} weights do not describe k centres over {F} planes")
        pe = None
        if plane_exp is not None:
            pe = np.ascontiguousarray(plane_exp, dtype=np.int32).reshape(-1)
            if pe.size != F:
                raise ValueError(f"isodata_sweep: {pe.size} plane exponents for {F} planes")
        k, cols = centers.shape[0], 1 + 2 * F
        table = self.empty(k * cols, torch.int64) if want_table else None
        changed, left = C.c_int64(0), C.c_int64(0)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.rsseg_isodata_sweep(self.h, self._pp(planes), F, L.F32 if dt == torch.float32 else L.U8, n,
                                               None if mask is None else C.c_void_p(mask.data_ptr()),
                                               None if pe is None else pe.ctypes.data_as(C.POINTER(C.c_int)), int(Q),
                                               weight.ctypes.data_as(dp), k, centers.ctypes.data_as(dp),
                                               C.c_void_p(labels.data_ptr()) if n else None,
                                               C.c_void_p(table.data_ptr()) if want_table else None, C.byref(changed), C.byref(left)))
        return (table.reshape(k, cols) if want_table else None), changed.value, left.value

    # ---- K29: Gaussian mixture (rsseg/gmm.py) ---------------------------------------------------------
    def gmm_plan(self, F: int, k: int, u8: bool = False, diag: bool = False) -> Tuple[int, int]:
        """(path, tile_pixels) of rsseg_gmm_sweep for F planes and k components: path 0 keeps the workgroup's table in LDS,
        1 adds into the global table."""
        path, tile = C.c_int(0), C.c_int(0)
        self.lib.rsseg_gmm_plan(int(F), int(k), L.U8 if u8 else L.F32, int(bool(diag)), C.byref(path), C.byref(tile))
        return path.value, tile.value

    def gmm_sweep(self, planes: Sequence, model, mask=None, want_table: bool = True, want_labels: bool = False, want_posterior: bool = False,
                  want_loglik: bool = False, want_proba: bool = False):
        """rsseg_gmm_sweep (include/rsseg.h) on flat float32 or uint8 device planes.  model: a dict of mean (k, F), whiten
        (k, F (F + 1) / 2), offset (k,) in u units, plane_exp (F ints; None for uint8 planes), Q, diag (bool).  -> a dict of
        table (int64 device [k, columns] or None), labels (uint8), posterior, loglik (float32), proba (float32 [k, n]), each
        None unless wanted, and the ints n_counted, n_left_out, n_far, ll_sum.  mask: None or a uint8 plane, 0 = not counted."""
        torch = _torch()
        F = len(planes)
        if F == 0:
            raise ValueError("gmm_sweep: no feature planes")
        dt, n = planes[0].dtype, planes[0].numel()
        if any(p.dtype != dt or p.numel() != n for p in planes) or dt not in (torch.float32, torch.uint8):
            raise ValueError("gmm_sweep: planes must all be float32 or all uint8, of one length")
        if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != n):
            raise ValueError("gmm_sweep: mask must be a uint8 plane of the planes' length")
        mean = np.ascontiguousarray(model["mean"], dtype=np.float64)
        offset = np.ascontiguousarray(model["offset"], dtype=np.float64).reshape(-1)
        k = offset.size
        whiten = np.ascontiguousarray(model["whiten"], dtype=np.float64).reshape(k, -1) if k else np.zeros((0, 0))
        if mean.ndim != 2 or mean.shape != (k, F) or whiten.shape != (k, F * (F + 1) // 2):
            raise ValueError(f"gmm_sweep: the model's shapes (mean {mean.shape}, whiten {whiten.shape}, offset {offset.shape}) do not "
                             f"describe k components over the call's {F} planes")
        pe = None
        if model.get("plane_exp") is not None:
            pe = np.ascontiguousarray(model["plane_exp"], dtype=np.int32).reshape(-1)
            if pe.size != F:
                raise ValueError(f"gmm_sweep: {pe.size} plane exponents for {F} planes")
        diag = bool(model.get("diag", False))
        cols = 1 + 2 * F if diag else 1 + F + F * (F + 1) // 2
        table = self.empty(max(k, 1) * cols, torch.int64) if want_table else None
        labels = self.empty(max(n, 1), torch.uint8) if want_labels else None
        posterior = self.empty(max(n, 1), torch.float32) if want_posterior else None
        loglik = self.empty(max(n, 1), torch.float32) if want_loglik else None
        proba = self.empty(max(n * k, 1), torch.float32) if want_proba else None
        tail = (C.c_int64 * 4)()
        dp = C.POINTER(C.c_double)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        self._chk(self.lib.rsseg_gmm_sweep(self.h, self._pp(planes), F, L.F32 if dt == torch.float32 else L.U8, n, ptr(mask),
                                           None if pe is None else pe.ctypes.data_as(C.POINTER(C.c_int)), int(model["Q"]), k, int(diag),
                                           mean.ctypes.data_as(dp), whiten.ctypes.data_as(dp), offset.ctypes.data_as(dp), ptr(table),
                                           ptr(labels), ptr(posterior), ptr(loglik), ptr(proba), tail))
        return dict(table=table.reshape(max(k, 1), cols)[:k] if want_table else None, labels=labels[:n] if want_labels else None,
                    posterior=posterior[:n] if want_posterior else None, loglik=loglik[:n] if want_loglik else None,
                    proba=proba[:n * k].reshape(k, n) if want_proba else None, n_counted=int(tail[0]), n_left_out=int(tail[1]),
                    n_far=int(tail[2]), ll_sum=int(tail[3]))

    # ---- K11 -----------------------------------------------------------------------------------
    def forest_load(self, forest: dict):
        f = forest
        ip, lp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
        keep = [np.ascontiguousarray(f["tree_off"], np.int64), np.ascontiguousarray(f["left"], np.int32),
                np.ascontiguousarray(f["right"], np.int32), np.ascontiguousarray(f["feature"], np.int32),
                np.ascontiguousarray(f["threshold"], np.float64), np.ascontiguousarray(f["missing_left"], np.uint8),
                np.ascontiguousarray(f["value"], np.float64), np.ascontiguousarray(f["classes"], np.int64)]
        self._chk(self.lib.rsseg_forest_load(self.h, len(keep[0]) - 1, keep[0].ctypes.data_as(lp), keep[1].ctypes.data_as(ip),
                                             keep[2].ctypes.data_as(ip), keep[3].ctypes.data_as(ip), keep[4].ctypes.data_as(dp),
                                             keep[5].ctypes.data_as(C.POINTER(C.c_uint8)), keep[6].ctypes.data_as(dp),
                                             keep[6].shape[1], keep[7].ctypes.data_as(lp), int(f["n_features"])))
        self._forest_shape = (len(keep[0]) - 1, int(keep[6].shape[1]), int(f["n_features"]))   # trees, classes, features

    def forest_predict(self, planes: Sequence):
        torch = _torch()
        n = planes[0].numel()
        out = self.empty(n, torch.int64)
        self._chk(self.lib.rsseg_forest_predict(self.h, self._pp(planes), len(planes), n, C.c_void_p(out.data_ptr())))
        return out

    def forest_predict_proba(self, planes: Sequence, proba: bool = True, confidence: bool = False, labels: bool = False):
        """rsseg_forest_predict_proba on the loaded forest, one launch for what is asked for.  Returns the device tensors
        (proba, confidence, labels), None for an output not asked for: proba float64 of shape (n_classes, n), class-planar
        (`.t()` is predict_proba's layout); confidence float64 (n,), the largest class probability; labels int64 (n,), what
        forest_predict returns."""
        torch = _torch()
        n = planes[0].numel()
        nc = getattr(self, "_forest_shape", (0, 1, 0))[1]   # without a forest the library refuses the call
        p = self.empty(nc * n, torch.float64) if proba else None
        c = self.empty(n, torch.float64) if confidence else None
        lab = self.empty(n, torch.int64) if labels else None
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        self._chk(self.lib.rsseg_forest_predict_proba(self.h, self._pp(planes), len(planes), n, ptr(p), ptr(c), ptr(lab)))
        return (None if p is None else p.view(nc, n)), c, lab

    def forest_oob(self, planes: Sequence, counts):
        """rsseg_forest_oob on the loaded forest over its training samples.  counts: int32 device tensor of n_trees * n
        bootstrap counts, tree after tree (what forest_fit takes).  Returns the device tensors (oob, n_oob): oob float64 of
        shape (n_classes, n), the leaf rows of the trees that never drew the sample summed in tree order and divided by
        max(n_oob, 1); n_oob int32 (n,), the number of those trees."""
        torch = _torch()
        n = planes[0].numel()
        nt, nc, _ = getattr(self, "_forest_shape", (0, 1, 0))
        if counts is not None and (counts.dtype != torch.int32 or counts.numel() != nt * n or not counts.is_contiguous()):
            raise ValueError(f"forest_oob: counts must be {nt} x {n} contiguous int32 values (one row per tree of the loaded forest)")
        oob = self.empty(nc * n, torch.float64)
        n_oob = self.empty(n, torch.int32)
        self._chk(self.lib.rsseg_forest_oob(self.h, self._pp(planes), len(planes), n, None if counts is None else C.c_void_p(counts.data_ptr()),
                                            C.c_void_p(oob.data_ptr()), C.c_void_p(n_oob.data_ptr())))
        return oob.view(nc, n), n_oob

    def forest_permutation_counts(self, planes: Sequence, y, src, jobs) -> np.ndarray:
        """rsseg_forest_permutation_counts on the loaded forest: for every record of `jobs` (dtype rsseg._lib.PERM_JOB: feature,
        source) the number of samples whose label index equals y when feature `feature` of every sample i is taken from row
        src[source, i] (feature -1: the samples as they are).  planes: F float32 device planes of n samples; y: int32 device
        class indices, -1 for a label the forest does not know; src: int32 device tensor of whole rows of n sample indices
        (None when no job substitutes).  One launch and one wait for all jobs; returns int64 counts, one per job.  ValueError
        with the library's message for what it refuses (a source index outside [0, n) among them)."""
        torch = _torch()
        n = planes[0].numel()
        jobs = np.ascontiguousarray(jobs, np.dtype(L.PERM_JOB)).reshape(-1)
        if y is not None and (y.dtype != torch.int32 or y.numel() != n or not y.is_contiguous()):
            raise ValueError(f"forest_permutation_counts: y must be {n} contiguous int32 class indices")
        n_src = 0
        if src is not None:
            if src.dtype != torch.int32 or not src.is_contiguous() or (n and src.numel() % n):
                raise ValueError(f"forest_permutation_counts: src must hold whole rows of {n} contiguous int32 sample indices")
            n_src = src.numel() // n if n else 0
        counts = np.zeros(len(jobs), np.int64)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        self._chk(self.lib.rsseg_forest_permutation_counts(self.h, self._pp(planes), len(planes), n, ptr(y), ptr(src), n_src,
                                                           jobs.ctypes.data_as(C.c_void_p), len(jobs),
                                                           counts.ctypes.data_as(C.POINTER(C.c_int64))))
        return counts

    # ---- K16 -----------------------------------------------------------------------------------
    def forest_fit(self, planes: Sequence, y, counts, seeds: np.ndarray, node_caps: np.ndarray, max_depth: int,
                   min_samples_split: int, min_samples_leaf: int, max_features: int, n_classes: int) -> List[dict]:
        """rsseg_forest_fit: grows one tree per entry of `seeds` on the device.  planes: F float32 device planes of n samples;
        y: int32 device class indices; counts: int32 device bootstrap counts, (n_trees * n) or one shared row of n, every row
        non-negative and summing to n (ValueError otherwise: weighted_n_samples is taken as n);
        node_caps[t] = 2 m_t - 1 (m_t = samples of tree t with a non-zero count).  Returns per tree a dict of NumPy arrays
        (left, right, feature, threshold, impurity, n_node_samples, weighted_n_node_samples, missing_go_to_left, value of
        shape (nodes, C)) and the tree's max_depth."""
        same = counts.numel() == planes[0].numel()
        seeds = np.ascontiguousarray(seeds, np.uint32)
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

        def call(n, off, out, nc, md):
            return self.lib.rsseg_forest_fit(self.h, self._pp(planes), len(planes), n, vp(y), int(n_classes), vp(counts), int(same), len(seeds),
                                             seeds.ctypes.data_as(C.POINTER(C.c_uint32)), int(max_depth), int(min_samples_split),
                                             int(min_samples_leaf), int(max_features), off, *out, nc, md)
        return self._forest_grow(call, planes[0].numel(), node_caps, n_classes)

    def forest_fit_jobs(self, planes: Sequence, y, counts, jobs: np.ndarray, node_caps: np.ndarray, n_classes: int) -> List[dict]:
        """rsseg_forest_fit_jobs: grows one tree per record of `jobs` (dtype rsseg._lib.FOREST_JOB: counts_row, weight_total, seed,
        max_depth, min_samples_split, min_samples_leaf, max_features) in one call.  counts: int32 device tensor of whole rows of
        n counts; tree t reads row jobs[t].counts_row, which is non-negative and sums to jobs[t].weight_total (ValueError
        otherwise), and trees may share rows.  planes, y, node_caps and the result: as forest_fit."""
        n = planes[0].numel()
        if counts.numel() == 0 or counts.numel() % n:
            raise ValueError(f"forest_fit_jobs: counts must hold whole rows of {n} values")
        jobs = np.ascontiguousarray(jobs, np.dtype(L.FOREST_JOB))
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

        def call(n, off, out, nc, md):
            return self.lib.rsseg_forest_fit_jobs(self.h, self._pp(planes), len(planes), n, vp(y), int(n_classes), vp(counts), counts.numel() // n,
                                                  len(jobs), jobs.ctypes.data_as(C.c_void_p), off, *out, nc, md)
        return self._forest_grow(call, n, node_caps, n_classes)

    def _forest_grow(self, call, n: int, node_caps: np.ndarray, n_classes: int) -> List[dict]:
        """Node storage for trees of `node_caps` records, the library call `call(n, node_off, node arrays, node_count,
        max_depth)`, and the nodes that were built, copied back per tree."""
        torch = _torch()
        T = len(node_caps)
        off = np.zeros(T + 1, np.int64)
        off[1:] = np.cumsum(np.asarray(node_caps, np.int64))
        total = int(off[-1])
        i32 = lambda k=1: self.empty(total * k, torch.int32)   # noqa: E731
        left, right, feat, n_node, w_node = i32(), i32(), i32(), i32(), i32()
        thr, imp = self.empty(total, torch.float64), self.empty(total, torch.float64)
        miss = self.empty(total, torch.uint8)
        value = self.empty(total * n_classes, torch.float64)
        nc = np.zeros(T, np.int64)
        md = np.zeros(T, np.int32)
        out = [C.c_void_p(t.data_ptr()) for t in (left, right, feat, thr, imp, n_node, w_node, miss, value)]
        self._chk(call(n, off.ctypes.data_as(C.POINTER(C.c_int64)), out, nc.ctypes.data_as(C.POINTER(C.c_int64)),
                       md.ctypes.data_as(C.POINTER(C.c_int32))))
        # copy back only the nodes that were built
        keep = np.concatenate([np.arange(off[t], off[t] + nc[t]) for t in range(T)]) if T else np.zeros(0, np.int64)
        idx = torch.from_numpy(keep).to(self.device)
        host = {k: v.index_select(0, idx).cpu().numpy() for k, v in
                (("left", left), ("right", right), ("feature", feat), ("threshold", thr), ("impurity", imp),
                 ("n_node_samples", n_node), ("weighted_n_node_samples", w_node), ("missing_go_to_left", miss))}
        host["value"] = value.view(total, n_classes).index_select(0, idx).cpu().numpy()
        trees, pos = [], 0
        for t in range(T):
            k = int(nc[t])
            trees.append({key: a[pos:pos + k] for key, a in host.items()})
            trees[-1]["max_depth"] = int(md[t])
            pos += k
        return trees

    # ---- K14 -----------------------------------------------------------------------------------
    def confusion_counts(self, truth, pred, known_range: Optional[Sequence[int]] = None):
        """rsseg_confusion_counts: the joint count table of (truth, pred) over the pixels where truth > 0.  truth, pred: device
        tensors of equal length (truth uint8 / int16 / uint16 / int32 / int64, pred uint8 / int32 / int64).  known_range:
        (tmin, tmax, pmin, pmax) that holds every valid pixel, or None for the range pass.  Returns (truth_values, pred_values,
        table): the sorted values of the non-empty rows and columns in the input dtypes and the int64 table restricted to
        them (empty when no pixel is valid).  A table beyond EVAL_MAX_CELLS raises RssegUnsupported."""
        torch = _torch()
        codes = {torch.uint8: L.U8, torch.int16: L.I16, torch.uint16: L.U16, torch.int32: L.I32, torch.int64: L.I64}
        if truth.dtype not in codes or pred.dtype not in (torch.uint8, torch.int32, torch.int64):
            raise ValueError(f"confusion_counts: truth {truth.dtype} / prediction {pred.dtype} not supported")
        if truth.numel() != pred.numel():
            raise ValueError(f"confusion_counts: {truth.numel()} truth values, {pred.numel()} predictions")
        planes = []
        for t in (truth.reshape(-1), pred.reshape(-1)):
            if t.data_ptr() % 16 or not t.is_contiguous():   # the kernels read 16-byte vectors from an aligned start
                t = t.clone(memory_format=torch.contiguous_format)
            planes.append(t)
        t, p = planes
        kr = None if known_range is None else (C.c_int64 * 4)(*[int(v) for v in known_range])
        rng = (C.c_int64 * 4)()
        nv = C.c_int64(0)
        cap = L.EVAL_MAX_CELLS
        counts = np.zeros(cap, np.int64)
        self._chk(self.lib.rsseg_confusion_counts(self.h, C.c_void_p(t.data_ptr()), codes[t.dtype], C.c_void_p(p.data_ptr()), codes[p.dtype],
                                                  t.numel(), kr, rng, C.byref(nv), counts.ctypes.data_as(C.POINTER(C.c_int64)), cap))
        tnp, pnp = np.dtype(str(t.dtype).split(".")[1]), np.dtype(str(p.dtype).split(".")[1])
        tmin, tmax, pmin, pmax = rng[:]
        if nv.value == 0:
            return np.zeros(0, tnp), np.zeros(0, pnp), np.zeros((0, 0), np.int64)
        nt, npv = tmax - tmin + 1, pmax - pmin + 1
        table = counts[:nt * npv].reshape(nt, npv)
        rows, cols = np.flatnonzero(table.sum(1)), np.flatnonzero(table.sum(0))
        return ((tmin + rows).astype(tnp), (pmin + cols).astype(pnp), np.ascontiguousarray(table[np.ix_(rows, cols)]))

    # ---- K15 -----------------------------------------------------------------------------------
    def _dn_code(self, t, what: str) -> int:
        torch = _torch()
        codes = {torch.uint8: L.U8, torch.int16: L.I16, torch.uint16: L.U16, torch.int32: L.I32, torch.float32: L.F32,
                 torch.float64: L.F64}
        if t.dtype not in codes:
            raise ValueError(f"{what}: input dtype {str(t.dtype).split('.')[-1]} not supported "
                             "(uint8, int16, uint16, int32, float32 or float64)")
        return codes[t.dtype]

    @staticmethod
    def _aligned(t):
        t = t.reshape(-1)
        if t.data_ptr() % 16 or not t.is_contiguous():   # the kernels read 16-byte vectors from an aligned start
            t = t.clone(memory_format=_torch().contiguous_format)
        return t

    def preprocess_u8(self, planes: Sequence, gain: Optional[Sequence[float]] = None, bias: Optional[Sequence[float]] = None,
                      want_range: bool = False, out: Optional[Sequence] = None):
        """rsseg_preprocess_u8: calibration (gain * DN + bias), identity warp and min-max stretch to uint8 of equal-length
        device planes of one dtype, without a host wait.  gain / bias None: the stretch alone.  Returns the uint8 planes, and
        with want_range also the whole raster's (n_bands, 3) float64 array {min, max of the non-NaN DN, NaN count} (one host
        wait)."""
        torch = _torch()
        if not planes:
            raise ValueError("preprocess_u8: no planes")
        code = self._dn_code(planes[0], "preprocess_u8")
        if any(p.dtype != planes[0].dtype or p.numel() != planes[0].numel() for p in planes):
            raise ValueError("preprocess_u8: the planes must share one dtype and length")
        ins = [self._aligned(p) for p in planes]
        n, nb = ins[0].numel(), len(ins)
        outs = list(out) if out is not None else [self.empty(n, torch.uint8) for _ in range(nb)]
        if len(outs) != nb or any(o.dtype != torch.uint8 or o.numel() != n or o.data_ptr() % 16 or not o.is_contiguous() for o in outs):
            raise ValueError("preprocess_u8: out must hold one contiguous, 16-byte aligned uint8 plane per band")
        if self._needs_keep():
            self._keep.extend(ins)
        g = b = None
        if gain is not None or bias is not None:
            if gain is None or bias is None or len(gain) != nb or len(bias) != nb:
                raise ValueError("preprocess_u8: gain and bias need one value per band each")
            g, b = (C.c_double * nb)(*[float(v) for v in gain]), (C.c_double * nb)(*[float(v) for v in bias])
        rng = np.zeros((nb, 3), np.float64) if want_range else None
        self._chk(self.lib.rsseg_preprocess_u8(self.h, self._pp(ins), code, nb, n, g, b, self._pp(outs),
                                               None if rng is None else rng.ctypes.data_as(C.POINTER(C.c_double))))
        return (outs, rng) if want_range else outs

    def radiometric(self, plane, gain: float, bias: float, out=None):
        """rsseg_radiometric: gain * plane + bias, float64 (float32 for a float32 plane), as NumPy 2 computes it."""
        torch = _torch()
        code = self._dn_code(plane, "radiometric")
        x = self._aligned(plane)
        dt = torch.float32 if x.dtype == torch.float32 else torch.float64
        out = out if out is not None else self.empty(x.numel(), dt)
        if out.dtype != dt or out.numel() != x.numel() or not out.is_contiguous():
            raise ValueError(f"radiometric: out must be a contiguous {dt} plane of {x.numel()} values")
        self._chk(self.lib.rsseg_radiometric(self.h, C.c_void_p(x.data_ptr()), code, x.numel(), float(gain), float(bias),
                                             C.c_void_p(out.data_ptr())))
        return out

    # ---- K21 -----------------------------------------------------------------------------------
    WARP_METHODS = {"nearest": L.WARP_NEAREST, "bilinear": L.WARP_BILINEAR, "cubic": L.WARP_CUBIC}

    def warp_poly(self, planes: Sequence, H: int, W: int, coef, cx: float, cy: float, Ho: int, Wo: int, method: str = "nearest",
                  fill=0, out_dtype=None, want_mask: bool = True, out: Optional[Sequence] = None):
        """rsseg_warp_poly: the H x W device planes (one dtype out of K15's six, at most 16) resampled onto Ho x Wo planes
        at the source positions the two polynomials coef = (p0..p5, q0..q5) give (include/rsseg.h).  method: 'nearest',
        'bilinear' or 'cubic'; out_dtype: None (the planes' dtype), torch.float32 or torch.float64; fill: the value of
        the pixels that fall outside the source (it must be a value of an integer output dtype).  Returns
        (flat output planes, uint8 validity mask or None, n_valid).  `out`: planes to write instead of new ones."""
        torch = _torch()
        planes = list(planes)
        if not planes:
            raise ValueError("warp_poly: planes is empty")
        if len(planes) > L.WARP_MAX_BANDS:
            raise ValueError(f"warp_poly: planes holds {len(planes)} planes, at most {L.WARP_MAX_BANDS} are taken in one call")
        code = self._dn_code(planes[0], "warp_poly: planes")
        H, W, Ho, Wo = int(H), int(W), int(Ho), int(Wo)
        if any(p.dtype != planes[0].dtype or p.numel() != H * W for p in planes):
            raise ValueError(f"warp_poly: planes must share one dtype and hold H * W = {H} * {W} = {H * W} pixels each")
        if method not in self.WARP_METHODS:
            raise ValueError(f"warp_poly: method {method!r} is not one of 'nearest', 'bilinear', 'cubic'")
        odt = planes[0].dtype if out_dtype is None else out_dtype
        if odt != planes[0].dtype and odt not in (torch.float32, torch.float64):
            raise ValueError(f"warp_poly: out_dtype {odt} is neither the planes' dtype nor float32 / float64")
        ocode = code if odt == planes[0].dtype else (L.F32 if odt == torch.float32 else L.F64)
        c = np.ascontiguousarray(np.asarray(coef, np.float64).reshape(-1))
        if c.size != 12:
            raise ValueError(f"warp_poly: coef must hold 12 values (p0..p5, q0..q5), not {c.size}")
        ins = [p.reshape(-1) if p.is_contiguous() else p.contiguous().reshape(-1) for p in planes]
        n_out = Ho * Wo
        if Ho < 1 or Wo < 1:
            raise ValueError(f"warp_poly: Ho = {Ho}, Wo = {Wo}: both must be at least 1")
        outs = list(out) if out is not None else [self.empty(n_out, odt) for _ in ins]
        if len(outs) != len(ins) or any(o.dtype != odt or o.numel() != n_out or not o.is_contiguous() for o in outs):
            raise ValueError(f"warp_poly: out must hold one contiguous {odt} plane of Ho * Wo = {n_out} values per input plane")
        mask = self.empty(n_out, torch.uint8) if want_mask else None
        if self._needs_keep():
            self._keep.extend(ins)
        nv = C.c_int64(0)
        self._chk(self.lib.rsseg_warp_poly(self.h, self._pp(ins), code, len(ins), H, W, c.ctypes.data_as(C.POINTER(C.c_double)), float(cx),
                                           float(cy), self.WARP_METHODS[method], float(fill), self._pp(outs), ocode, Ho, Wo,
                                           None if mask is None else C.c_void_p(mask.data_ptr()), C.byref(nv)))
        return outs, mask, int(nv.value)


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    """Process-wide context on LOCAL_RANK (or device 0)."""
    global _default_ctx
    if _default_ctx is None:
        import os
        _default_ctx = Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _default_ctx


def host_kmeans_draws(n: int, k: int, dtype, seed: int = 42) -> Tuple[int, np.ndarray]:
    """CPU-only: the k-means++ random draws as the library computes them (for tests)."""
    lib = L.load()
    Lt = 2 + int(np.log(k))
    u = np.zeros(max((k - 1) * Lt, 1), np.float64)
    cid = C.c_int64(0)
    rc = lib.rsseg_host_kmeans_draws(seed, n, L.F32 if np.dtype(dtype) == np.float32 else L.F64, k, C.byref(cid),
                                     u.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != 0:
        raise ValueError("rsseg_host_kmeans_draws failed")
    return cid.value, u[:(k - 1) * Lt]
