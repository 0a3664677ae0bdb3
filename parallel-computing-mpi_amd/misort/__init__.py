"""misort -- MI355X-native bitonic sort (Python host mirror of the C-ABI).

Mirrors the reference's sorter interface, /root/reference/Parallel-Sorting/src/
psort.cc:

* ``parallel_bitonic_sort(buffer, loc_buf_size, max_size)``   (psort.cc:167)
* ``compare_split(local, recv, keep_max)``                    (psort.cc:116-164)
* ``check_sort(local_numbers, local_size)``                   (psort.cc:497-520)
* ``block_sizes(n, p)``                                       (psort.cc:556-562)

with MPI ranks replaced by GPUs (one process per GPU, RCCL over xGMI) and the
keys held in HBM as torch tensors.  Every call goes through libmisort.so
(hand-written gfx950 HIP kernels); there is no CPU fallback: a missing
extension raises ``NativeLibraryMissing``.
"""
import ctypes
import os

__all__ = [
    "U32", "U64", "F64", "F32", "MisortError", "NotPowerOfTwo", "NativeLibraryMissing",
    "library_path", "lib", "Context", "Group", "block_sizes", "schedule", "tile_log2", "plan",
    "sample_indices", "exchange_count", "set_shared_gpu_env", "rows_plan",
    "segment_class", "topk_plan", "topk_segments_plan",
]

U32, U64, F64 = 0, 1, 2
F32 = 3  # keys of the key-value sorts only (Context.sort_pairs, argsort, parallel_sort_pairs)
KIND_NAMES = ["tile_sort", "global_pass", "tile_merge", "merge_split", "other", "span_pass",
              "wide_pass", "run_merge", "exchange", "run_mergek", "run_mergek_kernel", "merge_split_tail"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("MISORT_LIBRARY") or os.path.join(os.path.dirname(_HERE), "lib", "libmisort.so")
_lib = None


class MisortError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"misort error {code}: {msg}")
        self.code = code


class NotPowerOfTwo(MisortError):
    """psort.cc:168-172: 'bitonic sort requires 2^d processors'."""


class NativeLibraryMissing(RuntimeError):
    pass


def library_path():
    return _LIB_PATH


def lib():
    """Load libmisort.so (built in-tree by parallel-computing-mpi_amd/csrc/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise NativeLibraryMissing(
            f"{_LIB_PATH} not built; run `make -C parallel-computing-mpi_amd/csrc` "
            "(or __graft_entry__.build())")
    L = ctypes.CDLL(_LIB_PATH)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    sig = {
        "misort_version": ([], i32),
        "misort_last_error": ([], ctypes.c_char_p),
        "misort_create": ([i32, ctypes.POINTER(vp)], i32),
        "misort_destroy": ([vp], i32),
        "misort_stream": ([vp], vp),
        "misort_synchronize": ([vp], i32),
        "misort_get_unique_id": ([vp], i32),
        "misort_comm_init": ([vp, i32, i32, vp], i32),
        "misort_comm_size": ([vp], i32),
        "misort_comm_rank": ([vp], i32),
        "misort_bitonic_schedule": ([i32, i32, vp, vp], i32),
        "misort_block_size": ([i64, i32, i32], i64),
        "misort_parallel_bitonic_sort": ([vp, i32, vp, i64, i64, vp], i32),
        "misort_parallel_bitonic_sort_oop": ([vp, i32, vp, vp, i64, i64, vp], i32),
        "misort_local_sort": ([vp, i32, vp, vp, i64, vp], i32),
        "misort_local_sort_pairs": ([vp, i32, vp, vp, vp, vp, i64, vp], i32),
        "misort_local_sort_pairs64": ([vp, i32, vp, vp, i32, vp, vp, i64, vp], i32),
        "misort_parallel_sort_pairs": ([vp, i32, vp, vp, vp, vp, i64, i64, vp], i32),
        "misort_local_sort_rows": ([vp, i32, vp, vp, i64, i64, vp], i32),
        "misort_local_sort_rows_pairs": ([vp, i32, vp, vp, vp, vp, i64, i64, vp], i32),
        "misort_rows_plan": ([i64, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32),
                              ctypes.POINTER(i32), i32], i32),
        "misort_local_topk_rows": ([vp, i32, vp, vp, vp, i64, i64, i64, i32, vp], i32),
        "misort_topk_plan": ([i64, i64, ctypes.POINTER(i32), i32], i32),
        "misort_local_sort_segments": ([vp, i32, vp, vp, i64, vp, i64, vp], i32),
        "misort_local_sort_segments_pairs": ([vp, i32, vp, vp, vp, vp, i64, vp, i64, vp], i32),
        "misort_local_topk_segments": ([vp, i32, vp, vp, vp, i64, vp, i64, i64, i32, vp], i32),
        "misort_topk_segments_plan": ([i64, i64, ctypes.POINTER(i32), i32], i32),
        "misort_segment_class": ([i64, i32], i32),
        "misort_merge_split": ([vp, i32, vp, i64, vp, i64, vp, i32, vp], i32),
        "misort_merge_split_tail": ([vp, i32, vp, i64, vp, i64, i32, vp], i32),
        "misort_parallel_quick_sort": ([vp, i32, vp, i64, vp, i64, ctypes.POINTER(i64), vp], i32),
        "misort_parallel_sample_sort": ([vp, i32, vp, vp, i64, i64, vp], i32),
        "misort_check_sort": ([vp, i32, vp, i64, ctypes.POINTER(i64), vp], i32),
        "misort_sort_host": ([vp, i32, vp, vp, i64, i64], i32),
        "misort_fill_splitmix": ([vp, i32, vp, i64, ctypes.c_uint64, i64, vp], i32),
        "misort_profile_enable": ([vp, i32], i32),
        "misort_profile_reset": ([vp], i32),
        "misort_profile_read": ([vp, i32, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_double),
                                 ctypes.POINTER(ctypes.c_double)], i32),
        "misort_tile_log2": ([i32], i32),
        "misort_profile_trace": ([vp, i32, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_double)], i32),
        "misort_profile_stage": ([vp, i32, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)], i32),
        "misort_plan": ([ctypes.c_int64, i32, ctypes.POINTER(i32), i32], i32),
        "misort_pass_probe": ([vp, i32, vp, vp, i64, i32, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_float)], i32),
        "misort_group_create": ([i32, ctypes.POINTER(vp)], i32),
        "misort_group_destroy": ([vp], i32),
        "misort_comm_init_group": ([vp, vp, i32], i32),
        "misort_set_full_exchange": ([vp, i32], i32),
        "misort_set_relay": ([vp, i32], i32),
        "misort_set_compress": ([vp, i32], i32),
        "misort_codec_probe": ([vp, i32, vp, i64, i32, ctypes.POINTER(ctypes.c_float),
                                ctypes.POINTER(ctypes.c_float), ctypes.POINTER(i64), vp], i32),
        "misort_exchange_raw_bytes": ([vp, ctypes.POINTER(i64)], i32),
        "misort_sample_stride": ([i64], i64),
        "misort_sample_count": ([i64], i64),
        "misort_exchange_count": ([i32, vp, i64, vp, i64], i64),
        "misort_exchange_stats": ([vp, ctypes.POINTER(i64), ctypes.POINTER(i64),
                                   ctypes.POINTER(i64)], i32),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def _check(rc):
    if rc < 0:
        msg = lib().misort_last_error().decode()
        if rc == -2:
            raise NotPowerOfTwo(rc, msg)
        raise MisortError(rc, msg)
    return rc


def block_sizes(n, p):
    """psort.cc:556-562 block layout."""
    return [int(lib().misort_block_size(n, p, r)) for r in range(p)]


def schedule(p, rank):
    """psort.cc:182-196: [(partner, keep_max)] per stage for `rank`."""
    partner = (ctypes.c_int * 64)()
    keep = (ctypes.c_int * 64)()
    s = _check(lib().misort_bitonic_schedule(p, rank, partner, keep))
    return [(partner[i], keep[i]) for i in range(s)]


def sample_indices(n):
    """Indices of the splitter samples of a sorted n-key block."""
    import numpy as np
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    S, C = int(lib().misort_sample_stride(n)), int(lib().misort_sample_count(n))
    return np.minimum(np.arange(C, dtype=np.int64) * S, n - 1)


def exchange_count(samples_min, n_min, samples_max, n_max):
    """k keys each side sends in a compare-split (-1 = whole blocks)."""
    import numpy as np
    a, b = np.ascontiguousarray(samples_min), np.ascontiguousarray(samples_max)
    dt = U32 if a.dtype == np.uint32 else U64
    return int(lib().misort_exchange_count(dt, a.ctypes.data_as(ctypes.c_void_p), n_min,
                                           b.ctypes.data_as(ctypes.c_void_p), n_max))


def set_shared_gpu_env(rank):
    """RCCL environment for ranks that share one GPU (see Context.comm_init_torch);
    call before the first RCCL call of the process."""
    os.environ["NCCL_HOSTID"] = f"misort-shared-gpu-rank{rank}"
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")


def tile_log2(key_bytes):
    return int(lib().misort_tile_log2(key_bytes))


def plan(n, key_bytes=4):
    """The HBM pass plan of a local sort of n keys: [(kind_name, hi, R, flip)]."""
    np_ = lib().misort_plan(n, key_bytes, None, 0)
    _check(np_ if np_ < 0 else 0)
    buf = (ctypes.c_int32 * (4 * max(np_, 1)))()
    lib().misort_plan(n, key_bytes, buf, np_)
    return [(KIND_NAMES[buf[4 * i]], buf[4 * i + 1], buf[4 * i + 2], bool(buf[4 * i + 3]))
            for i in range(np_)]


def rows_plan(cols, key_bytes=4):
    """How Context.sort_rows sorts rows of `cols` keys: ``{"path": "tile" (one
    SORT pass, 2^(tile_log2 - block_log2) rows per LDS tile) | "blocks" (rows
    padded to 2^block_log2 keys, then the passes of plan(2^block_log2)),
    "tile_log2", "block_log2", "passes": [(kind_name, hi, R, flip)]}``."""
    path, tile, block = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    refs = (ctypes.byref(path), ctypes.byref(tile), ctypes.byref(block))
    np_ = _check(lib().misort_rows_plan(cols, key_bytes, *refs, None, 0))
    buf = (ctypes.c_int32 * (4 * max(np_, 1)))()
    _check(lib().misort_rows_plan(cols, key_bytes, *refs, buf, np_))
    return {"path": ("tile", "blocks")[path.value], "tile_log2": tile.value, "block_log2": block.value,
            "passes": [(KIND_NAMES[buf[4 * i]], buf[4 * i + 1], buf[4 * i + 2], bool(buf[4 * i + 3]))
                       for i in range(np_)]}


def topk_plan(cols, k):
    """The passes of Context.topk_rows for rows of ``cols`` keys:
    ``[(m_in, LR, npieces, m_out)]``.  A pass cuts every row of m_in records into
    npieces blocks of 2^LR virtual records, sorts each in an LDS tile and keeps
    the first k: m_out = npieces * k records per row.  The first pass reads the
    keys, the last (npieces == 1) writes the outputs.  A (cols, k) that top-k
    does not take is a MisortError (code -1)."""
    np_ = _check(lib().misort_topk_plan(cols, k, None, 0))
    buf = (ctypes.c_int32 * (4 * max(np_, 1)))()
    _check(lib().misort_topk_plan(cols, k, buf, np_))
    # m_in reaches 2^31: stored as its unsigned 32-bit pattern
    return [(buf[4 * i] & 0xFFFFFFFF, buf[4 * i + 1], buf[4 * i + 2], buf[4 * i + 3]) for i in range(np_)]


def topk_segments_plan(len, k):
    """The passes of Context.topk_segments for ONE segment of ``len`` keys:
    ``[(m_in, LR, npieces, m_out)]`` as topk_plan gives them.  ``len == 0``: no
    pass (the fill alone writes the row); ``len <= 2^13``: one pass with
    ``LR = max(ceil_log2(len), 5)`` and ``m_out = min(len, k)``; longer: the
    passes of ``topk_plan(2^ceil_log2(len), k)``.  A (len, k) that the call
    refuses (k outside 1..2^13, len above 2^31, k > 1024 with len > 2^13) is a
    MisortError (code -1)."""
    np_ = _check(lib().misort_topk_segments_plan(len, k, None, 0))
    buf = (ctypes.c_int32 * (4 * max(np_, 1)))()
    _check(lib().misort_topk_segments_plan(len, k, buf, np_))
    # m_in reaches 2^31: stored as its unsigned 32-bit pattern
    return [(buf[4 * i] & 0xFFFFFFFF, buf[4 * i + 1], buf[4 * i + 2], buf[4 * i + 3]) for i in range(np_)]


def segment_class(len, key_bytes=4):
    """The class Context.sort_segments sorts a segment of ``len`` keys in: -1 for
    an empty one; up to 2^tile_log2(key_bytes) keys the row tile's block_log2,
    max(ceil_log2(len), 5); for longer ones ceil_log2(len), the block of the
    padded path.  For len >= 2 it is rows_plan(len, key_bytes)'s path and block."""
    if len < 0 or key_bytes not in (4, 8):
        raise ValueError(f"segment_class({len}, {key_bytes}): len >= 0 and key_bytes 4 or 8 are needed")
    return int(lib().misort_segment_class(len, key_bytes))


class Group:
    """In-process rank group: P ranks = P threads, one Context each (the
    exchange is a device-to-device copy; same schedule and merge-split as RCCL)."""

    def __init__(self, nranks):
        self._h = ctypes.c_void_p()
        _check(lib().misort_group_create(nranks, ctypes.byref(self._h)))
        self.nranks = nranks

    def close(self):
        if self._h:
            lib().misort_group_destroy(self._h)
            self._h = ctypes.c_void_p()

    def run(self, fn, devices=None):
        """Run fn(rank, ctx) on one thread per rank; returns the results."""
        import threading
        res, err = [None] * self.nranks, []
        ctxs = [Context((devices or [0])[r % len(devices or [0])]) for r in range(self.nranks)]
        for r, c in enumerate(ctxs):
            _check(lib().misort_comm_init_group(c._h, self._h, r))

        def body(r):
            try:
                import torch
                torch.cuda.set_device(ctxs[r].device)
                res[r] = fn(r, ctxs[r])
            except BaseException as e:  # noqa: BLE001 -- re-raised below
                err.append(e)

        th = [threading.Thread(target=body, args=(r,)) for r in range(self.nranks)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for c in ctxs:
            c.close()
        if err:
            raise err[0]
        return res


def _dtype_of(t):
    import torch
    m = {torch.int32: U32, torch.int64: U64, torch.float64: F64}
    if hasattr(torch, "uint32"):
        m[torch.uint32] = U32
    if hasattr(torch, "uint64"):
        m[torch.uint64] = U64
    if t.dtype not in m:
        raise TypeError(f"unsupported key dtype {t.dtype} (u32/u64/f64 keys)")
    return m[t.dtype]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _u32_storage(t):
    import torch
    return t.dtype == torch.int32 or (hasattr(torch, "uint32") and t.dtype == torch.uint32)


def _pair_key_dtype(keys):
    """Key type of the key-value sorts: uint32/int32 storage = u32, float32 = f32."""
    import torch
    if _u32_storage(keys):
        return U32
    if keys.dtype == torch.float32:
        return F32
    raise TypeError(f"unsupported key dtype {keys.dtype} (key-value sorts take u32/f32 keys)")


def _pair_values(values, what="values"):
    if values is not None and not _u32_storage(values):
        raise TypeError(f"unsupported {what} dtype {values.dtype} (uint32/int32 storage)")
    return values


def _pair64_key_dtype(keys):
    """Key type of the 64-bit key-value sort: uint64/int64 storage = u64, float64 = f64."""
    import torch
    if keys.dtype == torch.int64 or (hasattr(torch, "uint64") and keys.dtype == torch.uint64):
        return U64
    if keys.dtype == torch.float64:
        return F64
    raise TypeError(f"unsupported key dtype {keys.dtype} (sort_pairs64/argsort64 take u64/f64 keys)")


def _span_check(n, **tensors):
    """Every tensor given is contiguous and holds at least ``n`` elements
    (ValueError): the check of every local entry point.  None is skipped."""
    for name, t in tensors.items():
        if t is not None and (t.numel() < n or not t.is_contiguous()):
            raise ValueError(f"{name}: a contiguous tensor of at least {n} elements is needed, "
                             f"got {tuple(t.shape)} with strides {tuple(t.stride())}")


def _keys_check(ref, n, **tensors):
    """The checks of the keys-only entry points, tensor by tensor: each one given
    has ``ref``'s dtype (TypeError) and passes _span_check (ValueError).  None
    is skipped."""
    if n < 0:
        raise ValueError(f"negative element count {n}")
    for name, t in tensors.items():
        if t is None:
            continue
        if t.dtype != ref.dtype:
            raise TypeError(f"{name} is {t.dtype}, the keys are {ref.dtype}")
        _span_check(n, **{name: t})


class Context:
    """One GPU (HIP device) = one reference MPI rank.

    ``dtype`` of a tensor selects the key type: uint32/int32 storage = u32 keys,
    uint64/int64 storage = u64 keys (compared unsigned), float64 = f64 keys.

    ``stream=None`` is torch's current stream of the context's device; calls
    are asynchronous on their stream unless their docstring says otherwise.  A
    context's scratch buffers are shared by all its calls: calls on one stream
    need nothing, calls on different streams of one context must be ordered by
    the caller (an event or a wait); unordered ones are undefined.  A context
    is not thread-safe either: one per thread.
    """

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        _check(lib().misort_create(device, ctypes.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            lib().misort_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self, stream):
        if stream is None:
            import torch
            return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return ctypes.c_void_p(stream)

    # ---- communicator (MPI_COMM_WORLD -> RCCL) ---------------------------------
    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        _check(lib().misort_get_unique_id(buf))
        return buf.raw

    def comm_init(self, nranks, rank, uid):
        buf = ctypes.create_string_buffer(bytes(uid), 128)
        _check(lib().misort_comm_init(self._h, nranks, rank, buf))

    def comm_init_torch(self, group=None, share_gpu=None):
        """Create the RCCL communicator; the id travels over torch.distributed.

        share_gpu (default: env MISORT_SHARE_GPU=1): several ranks drive ONE
        GPU.  RCCL refuses two ranks on one device within a host, so each rank
        then presents its own host id (NCCL_HOSTID) and the ranks talk over
        RCCL's socket transport on loopback: the RCCL calls, schedule and
        merge-split are the production ones, the bandwidth is not xGMI's (a
        correctness mode for 1-GPU boxes, never a performance figure)."""
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        if share_gpu is None:
            share_gpu = os.environ.get("MISORT_SHARE_GPU", "0") == "1"
        if share_gpu and world > 1:
            set_shared_gpu_env(rank)
        obj = [self.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(obj, src=0, group=group)
        self.comm_init(world, rank, obj[0])

    @property
    def numprocs(self):
        return int(lib().misort_comm_size(self._h))

    @property
    def myid(self):
        return int(lib().misort_comm_rank(self._h))

    # ---- hot path ---------------------------------------------------------------
    def parallel_bitonic_sort(self, buffer, loc_buf_size=None, max_size=None, out=None,
                              stream=None):
        """psort.cc:167.  Sorts this rank's block `buffer[:loc_buf_size]` with the
        reference's hypercube schedule; returns the tensor holding the result
        (``buffer`` itself, or ``out`` when given: input left unchanged).
        Exactly the ``loc_buf_size`` keys of the block are written: the rest of
        a larger buffer, and everything around a view, stay as they were.  The
        tensors need element alignment only (a view that starts anywhere in its
        storage).  A non-contiguous tensor and one holding fewer than
        ``loc_buf_size`` elements raise ValueError, an ``out`` of another dtype
        TypeError."""
        loc = buffer.numel() if loc_buf_size is None else int(loc_buf_size)
        mx = 0 if max_size is None else int(max_size)  # 0: the largest block (collective)
        dt = _dtype_of(buffer)
        _keys_check(buffer, loc, buffer=buffer, out=out)
        if out is None:
            _check(lib().misort_parallel_bitonic_sort(self._h, dt, _ptr(buffer), loc, mx,
                                                      self._stream(stream)))
            return buffer
        _check(lib().misort_parallel_bitonic_sort_oop(self._h, dt, _ptr(buffer), _ptr(out), loc,
                                                      mx, self._stream(stream)))
        return out

    def parallel_quick_sort(self, buffer, loc_buf_size=None, out=None, stream=None):
        """psort.cc:377 (the reference binary's shipped sort).  Returns
        ``(out, n)``: this rank's sorted keys are ``out[:n]``, n data-dependent.
        ``out`` defaults to the reference's capacity, (loc+1)*P keys.  A
        non-contiguous tensor and a ``buffer`` of fewer than ``loc_buf_size``
        elements raise ValueError, an ``out`` of another dtype TypeError (an
        ``out`` too small for the result is MisortError, code -6)."""
        import torch
        loc = buffer.numel() if loc_buf_size is None else int(loc_buf_size)
        _keys_check(buffer, loc, buffer=buffer)
        _keys_check(buffer, 0, out=out)
        if out is None:
            out = torch.empty((loc + 1) * self.numprocs, dtype=buffer.dtype, device=buffer.device)
        n = ctypes.c_int64()
        _check(lib().misort_parallel_quick_sort(self._h, _dtype_of(buffer), _ptr(buffer), loc, _ptr(out),
                                                out.numel(), ctypes.byref(n), self._stream(stream)))
        return out, int(n.value)

    def parallel_sample_sort(self, buffer, loc_buf_size=None, max_size=None, out=None, stream=None):
        """psort.cc:203-375 redesigned (RCCL all-to-all).  Same contract as
        parallel_bitonic_sort: the globally sorted keys in the reference block
        layout, out of place (``out`` defaults to a new tensor).  A
        non-contiguous tensor and one holding fewer than ``loc_buf_size``
        elements raise ValueError, an ``out`` of another dtype TypeError."""
        import torch
        loc = buffer.numel() if loc_buf_size is None else int(loc_buf_size)
        mx = 0 if max_size is None else int(max_size)
        out = torch.empty_like(buffer) if out is None else out
        _keys_check(buffer, loc, buffer=buffer, out=out)
        _check(lib().misort_parallel_sample_sort(self._h, _dtype_of(buffer), _ptr(buffer), _ptr(out), loc, mx,
                                                 self._stream(stream)))
        return out

    def local_sort(self, inp, out=None, n=None, stream=None):
        """psort.cc:175 (std::sort of the local block) on the GPU: ``out[:n]`` =
        the first ``n`` keys of ``inp`` ascending (f64: -0.0 before +0.0,
        negative NaNs first, positive NaNs last, every key bit-exact).  The
        default sorts in place; with another ``out`` the input is left
        unchanged.  Exactly ``n`` elements are written.  The tensors need
        element alignment only (a view that starts anywhere in its storage).
        ``out`` is ``inp`` itself or does not overlap it: any other overlap of
        the two ``n``-key ranges is a MisortError (code -1).  A non-contiguous
        tensor and one holding fewer than ``n`` elements raise ValueError, an
        ``out`` of another dtype TypeError."""
        out = inp if out is None else out
        n = inp.numel() if n is None else int(n)
        _keys_check(inp, n, inp=inp, out=out)
        _check(lib().misort_local_sort(self._h, _dtype_of(inp), _ptr(inp), _ptr(out), n,
                                       self._stream(stream)))
        return out

    def sort_rows(self, inp, out=None, stream=None):
        """Sorts along the last dimension of a contiguous tensor of any rank >= 1:
        every row of ``shape[-1]`` keys ascending, on its own (u32/u64/f64 keys
        as in local_sort; f64: -0.0 before +0.0, negative NaNs first, positive
        NaNs last, every key bit-exact).  The default is a NEW tensor, the input
        is left unchanged; ``out=inp`` sorts in place and returns ``inp``.  Any
        other overlap of ``out`` with ``inp`` is a MisortError (code -1).  A
        non-contiguous tensor and a too-small ``out`` raise ValueError, an
        ``out`` of another dtype TypeError."""
        import torch
        dt = _dtype_of(inp)
        if inp.dim() < 1:
            raise ValueError("sort_rows needs a tensor of rank >= 1")
        out = torch.empty_like(inp) if out is None else out
        _keys_check(inp, inp.numel(), inp=inp, out=out)
        cols = inp.shape[-1]
        rows = inp.numel() // cols if cols else 0
        _check(lib().misort_local_sort_rows(self._h, dt, _ptr(inp), _ptr(out), rows, cols, self._stream(stream)))
        return out

    def sort_segments(self, inp, offsets, out=None, stream=None):
        """Sorts variable-length segments of the 1-D contiguous key tensor ``inp``
        (u32/u64/f64 keys as in local_sort), each ascending on its own:
        segment i is ``inp[offsets[i]:offsets[i + 1]]``.  ``offsets`` is a 1-D
        contiguous int64 tensor on ``inp``'s device with at least one element,
        non-decreasing, within [0, inp.numel()]; empty segments are allowed.
        The default is a NEW tensor (keys outside the segments are copied, the
        input is left unchanged); ``out=inp`` sorts in place and leaves the
        keys outside the segments alone.  Returns ``out``.

        The call waits once on the host for a kernel that validates and counts
        the segments (so it cannot be captured in a graph); malformed offsets
        are a MisortError (code -1) naming the first bad index, and nothing is
        written then.  Any overlap of ``out`` with ``inp`` other than
        ``out is inp``, or with ``offsets``, is a MisortError (code -1).  Wrong
        dtypes raise TypeError; wrong shapes, non-contiguous tensors, a
        too-small ``out`` and an ``offsets`` on another device ValueError."""
        import torch
        dt = _dtype_of(inp)
        if offsets.dtype != torch.int64:
            raise TypeError(f"offsets is {offsets.dtype}, int64 is needed")
        if inp.dim() != 1:
            raise ValueError(f"sort_segments needs a 1-D key tensor, got {tuple(inp.shape)}")
        if offsets.dim() != 1 or offsets.numel() < 1 or not offsets.is_contiguous():
            raise ValueError("offsets: a contiguous 1-D tensor of at least one element is needed, "
                             f"got {tuple(offsets.shape)} with strides {tuple(offsets.stride())}")
        if offsets.device != inp.device:
            raise ValueError(f"offsets is on {offsets.device}, the keys are on {inp.device}")
        out = torch.empty_like(inp) if out is None else out
        n = inp.numel()
        _keys_check(inp, n, inp=inp, out=out)
        if out.device != inp.device:
            raise ValueError(f"out is on {out.device}, the keys are on {inp.device}")
        _check(lib().misort_local_sort_segments(self._h, dt, _ptr(inp), _ptr(out), n, _ptr(offsets),
                                                offsets.numel() - 1, self._stream(stream)))
        return out

    # ---- key-value sort ----------------------------------------------------------
    def _pair_outputs(self, keys, values, out_keys, out_values, n):
        import torch
        if out_values is None:  # indices of float keys: 32-bit integers of the keys' shape
            like = values if values is not None else keys
            out_values = torch.empty_like(like) if _u32_storage(like) else torch.empty_like(like, dtype=torch.int32)
        _pair_values(out_values, "out_values")
        if out_keys is not None and out_keys.dtype != keys.dtype:
            raise TypeError(f"out_keys is {out_keys.dtype}, the keys are {keys.dtype}")
        _span_check(n, keys=keys, values=values, out_keys=out_keys, out_values=out_values)
        return out_values

    def sort_pairs(self, keys, values=None, out_keys=None, out_values=None, n=None, stream=None):
        """Key-value sort on this GPU: the pairs ascending by (key, value), values
        compared unsigned.  Keys are u32 (uint32/int32 storage) or float32 (total
        order of the bit patterns: -0.0 before +0.0, negative NaNs first, positive
        NaNs last); values are uint32/int32 storage.  ``values=None``: the value
        of element i is i.  Outputs may be the inputs.  Returns ``(out_keys,
        out_values)``."""
        import torch
        dt = _pair_key_dtype(keys)
        _pair_values(values)
        n = keys.numel() if n is None else int(n)
        out_keys = torch.empty_like(keys) if out_keys is None else out_keys
        out_values = self._pair_outputs(keys, values, out_keys, out_values, n)
        _check(lib().misort_local_sort_pairs(self._h, dt, _ptr(keys), _ptr(values) if values is not None else None,
                                             _ptr(out_keys), _ptr(out_values), n, self._stream(stream)))
        return out_keys, out_values

    def argsort(self, keys, out=None, n=None, stream=None):
        """The stable argsort of u32 or float32 keys (order as in sort_pairs):
        ``out[j]`` is the index of the j-th smallest key, equal keys in input
        order.  No keys are written.  ``out`` is uint32/int32 storage (default:
        a new tensor like u32 keys, int32 for float keys); the indices are
        unsigned 32-bit patterns."""
        dt = _pair_key_dtype(keys)
        n = keys.numel() if n is None else int(n)
        out = self._pair_outputs(keys, None, None, out, n)
        _check(lib().misort_local_sort_pairs(self._h, dt, _ptr(keys), None, None, _ptr(out), n,
                                             self._stream(stream)))
        return out

    def _rows_pairs_shape(self, what, keys, values=None):
        """(rows, cols) of the row-wise key-value sorts; the checks sort_rows makes."""
        if keys.dim() < 1:
            raise ValueError(f"{what} needs a tensor of rank >= 1")
        if not keys.is_contiguous():
            raise ValueError(f"{what} needs a contiguous tensor, got strides {tuple(keys.stride())}")
        if values is not None and values.shape != keys.shape:
            raise ValueError(f"values have shape {tuple(values.shape)}, the keys {tuple(keys.shape)}")
        cols = keys.shape[-1]
        return (keys.numel() // cols if cols else 0), cols

    def sort_rows_pairs(self, keys, values=None, out_keys=None, out_values=None, stream=None):
        """Key-value sort along the last dimension of contiguous tensors of any
        rank >= 1: every row of ``shape[-1]`` pairs on its own, ascending by
        (key, value), values compared unsigned: the order of sort_pairs, row by
        row.  Keys are u32 (uint32/int32 storage) or float32 (total order of the
        bit patterns: -0.0 before +0.0, negative NaNs first, positive NaNs last,
        every key bit-exact); values are uint32/int32 storage of the keys'
        shape.  ``values=None``: the value of a row's column c is c, so
        ``out_values`` is the stable row-wise argsort (equal keys in column
        order).  These are 32-bit indices where torch.sort returns int64.
        The default outputs are NEW tensors and the inputs are left unchanged.
        ``out_keys=keys`` and ``out_values=values`` sort in place; any other
        overlap among the four tensors is a MisortError (code -1).  A
        non-contiguous tensor, rank 0, a too-small output and a ``values`` of
        another shape raise ValueError, wrong dtypes TypeError.  Returns
        ``(out_keys, out_values)``."""
        import torch
        dt = _pair_key_dtype(keys)
        _pair_values(values)
        rows, cols = self._rows_pairs_shape("sort_rows_pairs", keys, values)
        out_keys = torch.empty_like(keys) if out_keys is None else out_keys
        out_values = self._pair_outputs(keys, values, out_keys, out_values, keys.numel())
        _check(lib().misort_local_sort_rows_pairs(self._h, dt, _ptr(keys),
                                                  _ptr(values) if values is not None else None, _ptr(out_keys),
                                                  _ptr(out_values), rows, cols, self._stream(stream)))
        return out_keys, out_values

    def argsort_rows(self, keys, out=None, stream=None):
        """The stable argsort along the last dimension of a contiguous tensor of
        u32 or float32 keys (order as in sort_rows_pairs): ``out[..., j]`` is the
        column of the row's j-th smallest key, equal keys in column order.  No
        keys are written.  ``out`` is uint32/int32 storage (default: a new tensor
        of the keys' shape, like u32 keys, int32 for float keys): 32-bit indices
        where torch.argsort returns int64.  ``out`` must not overlap ``keys``
        (MisortError, code -1)."""
        dt = _pair_key_dtype(keys)
        rows, cols = self._rows_pairs_shape("argsort_rows", keys)
        out = self._pair_outputs(keys, None, None, out, keys.numel())
        _check(lib().misort_local_sort_rows_pairs(self._h, dt, _ptr(keys), None, None, _ptr(out), rows, cols,
                                                  self._stream(stream)))
        return out

    def _segments_pairs_check(self, what, keys, offsets, **others):
        """The shape and device checks of the segmented key-value sorts (those
        of sort_segments); returns the number of segments."""
        import torch
        if offsets.dtype != torch.int64:
            raise TypeError(f"offsets is {offsets.dtype}, int64 is needed")
        if keys.dim() != 1:
            raise ValueError(f"{what} needs a 1-D key tensor, got {tuple(keys.shape)}")
        if offsets.dim() != 1 or offsets.numel() < 1 or not offsets.is_contiguous():
            raise ValueError("offsets: a contiguous 1-D tensor of at least one element is needed, "
                             f"got {tuple(offsets.shape)} with strides {tuple(offsets.stride())}")
        if offsets.device != keys.device:
            raise ValueError(f"offsets is on {offsets.device}, the keys are on {keys.device}")
        for name, t in others.items():
            if t is not None and t.device != keys.device:
                raise ValueError(f"{name} is on {t.device}, the keys are on {keys.device}")
        return offsets.numel() - 1

    def sort_segments_pairs(self, keys, offsets, values=None, out_keys=None, out_values=None, stream=None):
        """Key-value sort of variable-length segments of the 1-D contiguous
        tensors ``keys`` and ``values``: segment i is the pairs
        ``[offsets[i], offsets[i + 1])``, sorted on its own, ascending by
        (key, value), values compared unsigned: the order of sort_rows_pairs,
        segment by segment.  Keys are u32 (uint32/int32 storage) or float32
        (total order of the bit patterns: -0.0 before +0.0, negative NaNs first,
        positive NaNs last, every key bit-exact); values are uint32/int32
        storage of the keys' shape.  ``offsets`` is as in sort_segments: a 1-D
        contiguous int64 tensor on the keys' device with at least one element,
        non-decreasing, within [0, keys.numel()]; empty segments are allowed.
        ``values=None``: the value of a pair is its position inside its segment,
        so ``out_values`` is the stable argsort of every segment (32-bit
        indices; ``keys[offsets[i] + idx]`` gathers the sorted segment); no
        segment may then be longer than 2^32 keys.

        The default outputs are NEW tensors and the inputs are left unchanged;
        pairs outside the segments are copied to the outputs that have an input
        (with ``values=None`` those elements of ``out_values`` are not written).
        ``out_keys=keys`` and ``out_values=values`` sort in place and leave the
        pairs outside the segments alone.  Any other overlap among the four
        tensors, or of an output with ``offsets``, is a MisortError (code -1).

        The call waits once on its stream: the host waits for a kernel that
        validates and counts the segments (so the call cannot be captured in a
        graph); malformed offsets are a MisortError (code -1) naming the first
        bad index, and nothing is written then.  Wrong dtypes raise TypeError;
        wrong shapes, non-contiguous tensors, a too-small output and a tensor on
        another device ValueError.  Returns ``(out_keys, out_values)``."""
        import torch
        dt = _pair_key_dtype(keys)
        _pair_values(values)
        nseg = self._segments_pairs_check("sort_segments_pairs", keys, offsets, values=values, out_keys=out_keys,
                                          out_values=out_values)
        if values is not None and values.shape != keys.shape:
            raise ValueError(f"values have shape {tuple(values.shape)}, the keys {tuple(keys.shape)}")
        out_keys = torch.empty_like(keys) if out_keys is None else out_keys
        out_values = self._pair_outputs(keys, values, out_keys, out_values, keys.numel())
        _check(lib().misort_local_sort_segments_pairs(self._h, dt, _ptr(keys),
                                                      _ptr(values) if values is not None else None, _ptr(out_keys),
                                                      _ptr(out_values), keys.numel(), _ptr(offsets), nseg,
                                                      self._stream(stream)))
        return out_keys, out_values

    def argsort_segments(self, keys, offsets, out=None, stream=None):
        """The stable argsort of every segment of the 1-D contiguous tensor of
        u32 or float32 keys (order and ``offsets`` as in sort_segments_pairs):
        ``out[offsets[i] + j]`` is the position, inside segment i, of the
        segment's j-th smallest key, equal keys in input order, so
        ``keys[offsets[i] + out[offsets[i] + j]]`` is that key.  No keys are
        written, and elements of ``out`` outside the segments are not written.
        ``out`` is uint32/int32 storage (default: a new tensor of the keys'
        shape, like u32 keys, int32 for float keys); it must not overlap
        ``keys`` or ``offsets`` (MisortError, code -1).  No segment may be
        longer than 2^32 keys.  The call waits once on its stream, as
        sort_segments_pairs does, and refuses malformed offsets the same way."""
        dt = _pair_key_dtype(keys)
        nseg = self._segments_pairs_check("argsort_segments", keys, offsets, out=out)
        out = self._pair_outputs(keys, None, None, out, keys.numel())
        _check(lib().misort_local_sort_segments_pairs(self._h, dt, _ptr(keys), None, None, _ptr(out), keys.numel(),
                                                      _ptr(offsets), nseg, self._stream(stream)))
        return out

    def _topk_out(self, name, out, like, dtype, shape, n):
        """An output of topk_rows: a new tensor of ``shape``, or the first n
        elements of the caller's tensor seen in that shape."""
        import torch
        if out is None:
            return torch.empty(shape, dtype=dtype, device=like.device)
        _span_check(n, **{name: out})
        if out.device != like.device:
            raise ValueError(f"{name} is on {out.device}, the keys are on {like.device}")
        return out if tuple(out.shape) == tuple(shape) else out.view(-1)[:n].view(shape)

    def topk_rows(self, keys, k, largest=True, out_values=None, out_indices=None, stream=None):
        """The k largest (``largest=True``) or smallest keys along the last
        dimension of a contiguous tensor of rank >= 1, and their columns:
        ``(values, indices)`` of shape ``keys.shape[:-1] + (k,)``, what
        ``torch.topk(keys, k, dim=-1, largest=largest, sorted=True)`` returns,
        without sorting the rows.  Keys are u32 (uint32/int32 storage, compared
        unsigned) or float32 in the total order of sort_rows_pairs (largest:
        positive NaNs first, then +inf ... +0.0, -0.0 ... -inf, negative NaNs
        last; smallest: the reverse), every value bit-exact.  Each row is sorted,
        best first; equal keys come out in ascending column order in both
        directions.  ``values`` has the keys' dtype, ``indices`` the storage of
        argsort_rows (like u32 keys, int32 for float keys): 32-bit columns where
        torch returns int64.  ``1 <= k <= shape[-1] <= 2^31``, and ``k <= 1024``
        for rows longer than 2^13 (else MisortError, code -1: use argsort_rows);
        ``k == 0`` gives empty outputs.  The outputs must not overlap the keys
        or each other (MisortError, code -1); the keys are left unchanged.  A
        non-contiguous tensor, rank 0, a negative k and a too-small output raise
        ValueError, wrong dtypes TypeError.  ``topk_plan(cols, k)`` tells the
        passes."""
        return self._topk_rows("topk_rows", keys, k, largest, True, out_values, out_indices, stream)

    def topk_rows_indices(self, keys, k, largest=True, out=None, stream=None):
        """The ``indices`` of topk_rows alone: no keys are written."""
        return self._topk_rows("topk_rows_indices", keys, k, largest, False, None, out, stream)[1]

    def _topk_rows(self, what, keys, k, largest, with_values, out_values, out_indices, stream):
        import torch
        dt = _pair_key_dtype(keys)
        rows, cols = self._rows_pairs_shape(what, keys)
        k = int(k)
        if k < 0:
            raise ValueError(f"{what}: negative k {k}")
        if out_values is not None and out_values.dtype != keys.dtype:
            raise TypeError(f"out_values is {out_values.dtype}, the keys are {keys.dtype}")
        _pair_values(out_indices, "out_indices")
        shape, n = tuple(keys.shape[:-1]) + (k,), rows * k
        values = self._topk_out("out_values", out_values, keys, keys.dtype, shape, n) if with_values else None
        indices = self._topk_out("out_indices", out_indices, keys,
                                 keys.dtype if _u32_storage(keys) else torch.int32, shape, n)
        _check(lib().misort_local_topk_rows(self._h, dt, _ptr(keys), _ptr(values) if with_values else None,
                                            _ptr(indices), rows, cols, k, 1 if largest else 0,
                                            self._stream(stream)))
        return values, indices

    def topk_segments(self, keys, offsets, k, largest=True, out_values=None, out_indices=None, stream=None):
        """The k largest (``largest=True``) or smallest keys of every segment of
        the 1-D contiguous tensor ``keys`` and their positions inside the
        segment: ``(values, indices)`` of shape ``(nseg, k)``, row i for segment
        i, the keys ``[offsets[i], offsets[i + 1])``.  ``offsets`` is as in
        sort_segments: a 1-D contiguous int64 tensor on the keys' device with at
        least one element, non-decreasing, within [0, keys.numel()]; empty
        segments are allowed and keys outside the segments are ignored.  Keys,
        order and ties are topk_rows': u32 (uint32/int32 storage, compared
        unsigned) or float32 in the total order of the bit patterns, each row
        sorted best first, equal keys in ascending position order in both
        directions, every real value bit-exact.  ``indices`` are the positions
        argsort_segments returns, in the storage of argsort_rows (like u32
        keys, int32 for float keys).

        Fill: a segment shorter than k (an empty one included) leaves the slots
        ``j >= len`` of its row with index 0xFFFFFFFF (-1 in int32 storage; a
        real position is below 2^31, so it marks absence) and the last key of
        the direction's order: u32 0xFFFFFFFF (smallest) or 0 (largest),
        float32 bit pattern 0x7FFFFFFF (smallest) or 0xFFFFFFFF (largest).  A
        real key may equal the fill key; only the index tells.

        ``1 <= k <= 2^13``, ``k <= 1024`` if any segment is longer than 2^13
        keys, and no segment may be longer than 2^31 keys (else MisortError,
        code -1, nothing written); ``k == 0`` gives empty outputs.  The outputs
        must not overlap the keys, the offsets or each other (MisortError, code
        -1); the inputs are left unchanged.

        The call waits once on its stream: the host waits for a kernel that
        validates and counts the segments (so the call cannot be captured in a
        graph); malformed offsets are a MisortError (code -1) naming the first
        bad index, and nothing is written then.  Wrong dtypes raise TypeError;
        wrong shapes, non-contiguous tensors, a negative k, a too-small output
        and a tensor on another device ValueError.  ``topk_segments_plan(len,
        k)`` tells the passes of one segment."""
        return self._topk_segments("topk_segments", keys, offsets, k, largest, True, out_values, out_indices, stream)

    def topk_segments_indices(self, keys, offsets, k, largest=True, out=None, stream=None):
        """The ``indices`` of topk_segments alone: no keys are written.  The
        fill index of a segment shorter than k is 0xFFFFFFFF (-1 in int32
        storage); the call waits once on its stream, as topk_segments does."""
        return self._topk_segments("topk_segments_indices", keys, offsets, k, largest, False, None, out, stream)[1]

    def _topk_segments(self, what, keys, offsets, k, largest, with_values, out_values, out_indices, stream):
        import torch
        dt = _pair_key_dtype(keys)
        nseg = self._segments_pairs_check(what, keys, offsets, out_values=out_values, out_indices=out_indices)
        if not keys.is_contiguous():
            raise ValueError(f"{what} needs a contiguous tensor, got strides {tuple(keys.stride())}")
        k = int(k)
        if k < 0:
            raise ValueError(f"{what}: negative k {k}")
        if out_values is not None and out_values.dtype != keys.dtype:
            raise TypeError(f"out_values is {out_values.dtype}, the keys are {keys.dtype}")
        _pair_values(out_indices, "out_indices")
        shape, n = (nseg, k), nseg * k
        values = self._topk_out("out_values", out_values, keys, keys.dtype, shape, n) if with_values else None
        indices = self._topk_out("out_indices", out_indices, keys,
                                 keys.dtype if _u32_storage(keys) else torch.int32, shape, n)
        _check(lib().misort_local_topk_segments(self._h, dt, _ptr(keys) if keys.numel() else None,
                                                _ptr(values) if with_values else None, _ptr(indices),
                                                keys.numel(), _ptr(offsets), nseg, k, 1 if largest else 0,
                                                self._stream(stream)))
        return values, indices

    def sort_pairs64(self, keys, values, out_keys=None, out_values=None, n=None, stream=None):
        """Stable key-value sort of 64-bit keys on this GPU: the pairs ascending
        by key, equal keys in input order (NOT sort_pairs' (key, value) order:
        the values are never compared).  Keys are u64 (uint64/int64 storage,
        compared unsigned) or float64 (order of local_sort: -0.0 before +0.0,
        negative NaNs first, positive NaNs last, every key bit-exact); values
        are any tensor of 4- or 8-byte elements, moved as bit patterns.
        ``out_keys`` may be ``keys``; no output may overlap ``values`` and the
        outputs must not overlap each other (MisortError, code -1).  Returns
        ``(out_keys, out_values)``."""
        import torch
        dt = _pair64_key_dtype(keys)
        if values.element_size() not in (4, 8):
            raise TypeError(f"unsupported values dtype {values.dtype} (4- or 8-byte elements)")
        n = keys.numel() if n is None else int(n)
        out_keys = torch.empty_like(keys) if out_keys is None else out_keys
        out_values = torch.empty_like(values) if out_values is None else out_values
        if out_keys.dtype != keys.dtype:
            raise TypeError(f"out_keys is {out_keys.dtype}, the keys are {keys.dtype}")
        if out_values.dtype != values.dtype:
            raise TypeError(f"out_values is {out_values.dtype}, the values are {values.dtype}")
        _span_check(n, keys=keys, values=values, out_keys=out_keys, out_values=out_values)
        _check(lib().misort_local_sort_pairs64(self._h, dt, _ptr(keys), _ptr(values), values.element_size(),
                                               _ptr(out_keys), _ptr(out_values), n, self._stream(stream)))
        return out_keys, out_values

    def argsort64(self, keys, out=None, n=None, stream=None):
        """The stable argsort of u64 or float64 keys (order as in sort_pairs64):
        ``out[j]`` is the index of the j-th smallest key, equal keys in input
        order.  No keys are written.  ``out`` is uint32/int32 storage (default:
        a new int32 tensor of the keys' shape); the indices are unsigned 32-bit
        patterns."""
        import torch
        dt = _pair64_key_dtype(keys)
        n = keys.numel() if n is None else int(n)
        out = torch.empty_like(keys, dtype=torch.int32) if out is None else out
        _pair_values(out, "out")
        _span_check(n, keys=keys, out=out)
        _check(lib().misort_local_sort_pairs64(self._h, dt, _ptr(keys), None, 4, None, _ptr(out), n,
                                               self._stream(stream)))
        return out

    def parallel_sort_pairs(self, keys, values=None, loc=None, max_size=None, out_keys=None, out_values=None,
                            stream=None):
        """sort_pairs over the communicator (the hypercube schedule of
        parallel_bitonic_sort): rank r ends with pairs [r*loc, (r+1)*loc) of the
        global (key, value) order.  Every rank passes the same ``loc`` (else every
        rank raises MisortError, code -1).  ``values=None``: the value is the
        global index rank*loc + i.  Returns ``(out_keys, out_values)``."""
        import torch
        dt = _pair_key_dtype(keys)
        _pair_values(values)
        loc = keys.numel() if loc is None else int(loc)
        mx = 0 if max_size is None else int(max_size)
        out_keys = torch.empty_like(keys) if out_keys is None else out_keys
        out_values = self._pair_outputs(keys, values, out_keys, out_values, loc)
        _check(lib().misort_parallel_sort_pairs(self._h, dt, _ptr(keys), _ptr(values) if values is not None else None,
                                                _ptr(out_keys), _ptr(out_values), loc, mx, self._stream(stream)))
        return out_keys, out_values

    def compare_split(self, local, recv, keep_max, out=None, stream=None, in_place_tail=False):
        """Device half of psort.cc:116-164 (no exchange).  in_place_tail: the
        small-bracket path of the hypercube stages (misort_merge_split_tail) on a
        copy of `local` in `out` (``out`` may be ``local`` itself: in place; the
        copy runs on ``stream`` like the merge, behind whatever is queued there).
        Exactly ``local.numel()`` elements of ``out`` are written; ``local`` (unless
        it is ``out``) and ``recv`` are left unchanged.  Without in_place_tail
        ``out`` must overlap neither ``local`` nor ``recv`` (MisortError, code
        -1).  The tensors need element alignment only.  A non-contiguous tensor
        and an ``out`` of fewer than ``local.numel()`` elements raise ValueError,
        a ``recv`` or ``out`` of another dtype TypeError."""
        import torch
        out = torch.empty_like(local) if out is None else out
        _keys_check(local, local.numel(), local=local, out=out)
        _keys_check(local, 0, recv=recv)
        if in_place_tail:
            if out.data_ptr() != local.data_ptr():
                # the copy is a step of the call: on `stream`, behind what is queued
                # there (which may still be writing `local`) and before the merge
                cur = torch.cuda.current_stream(local.device)
                if stream is not None and int(stream) != cur.cuda_stream:
                    with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=local.device)):
                        out[:local.numel()].copy_(local)
                else:
                    out[:local.numel()].copy_(local)
            _check(lib().misort_merge_split_tail(self._h, _dtype_of(local), _ptr(out), local.numel(),
                                                 _ptr(recv), recv.numel(), int(keep_max), self._stream(stream)))
            return out
        _check(lib().misort_merge_split(self._h, _dtype_of(local), _ptr(local), local.numel(),
                                        _ptr(recv), recv.numel(), _ptr(out), int(keep_max),
                                        self._stream(stream)))
        return out

    def check_sort(self, local_numbers, local_size=None, stream=None):
        """psort.cc:497-520: total error count over the communicator: every
        position i < local_size - 1 with a[i] > a[i+1] counts once (f64 compared
        as doubles: a NaN on either side is no descent), plus the descents
        between consecutive ranks' blocks.  The tensor is only read and needs
        element alignment only; a non-contiguous one, or one of fewer than
        ``local_size`` elements, raises ValueError."""
        n = local_numbers.numel() if local_size is None else int(local_size)
        _keys_check(local_numbers, n, local_numbers=local_numbers)
        err = ctypes.c_int64()
        _check(lib().misort_check_sort(self._h, _dtype_of(local_numbers), _ptr(local_numbers), n,
                                       ctypes.byref(err), self._stream(stream)))
        return int(err.value)

    def sort_host(self, arr, max_size=None, out=None):
        """numpy block -> pinned staging ring -> GPU parallel sort -> numpy
        (chunked and overlapped; `out` may be a preallocated array)."""
        import numpy as np
        arr = np.ascontiguousarray(arr)
        dt = {np.dtype(np.uint32): U32, np.dtype(np.uint64): U64,
              np.dtype(np.float64): F64}[arr.dtype]
        if out is None:
            out = np.empty_like(arr)
        elif out.dtype != arr.dtype or out.size < arr.size or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous array of the input dtype and size")
        mx = 0 if max_size is None else int(max_size)
        _check(lib().misort_sort_host(self._h, dt, arr.ctypes.data_as(ctypes.c_void_p),
                                      out.ctypes.data_as(ctypes.c_void_p), arr.size, mx))
        return out

    def fill_splitmix(self, out, seed, g0=0, stream=None):
        _check(lib().misort_fill_splitmix(self._h, _dtype_of(out), _ptr(out), out.numel(), seed, g0,
                                          self._stream(stream)))
        return out

    def synchronize(self):
        _check(lib().misort_synchronize(self._h))

    @property
    def native_stream(self):
        """The context's own hipStream_t (int), for stream=..."""
        return int(lib().misort_stream(self._h) or 0)

    def set_full_exchange(self, on=True):
        _check(lib().misort_set_full_exchange(self._h, int(on)))

    def set_relay(self, on=True):
        """Spread compare-split exchanges over every xGMI link (P > 2)."""
        _check(lib().misort_set_relay(self._h, int(on)))

    def set_compress(self, on=True):
        """Delta-code compare-split messages (lossless; default on)."""
        _check(lib().misort_set_compress(self._h, int(on)))

    def codec_probe(self, keys, decoded=None, reps=3):
        """Exchange codec on a sorted device run: (encode ms, decode ms, coded bytes)."""
        a, b, n = ctypes.c_float(), ctypes.c_float(), ctypes.c_int64()
        _check(lib().misort_codec_probe(self._h, _dtype_of(keys), _ptr(keys), keys.numel(), reps,
                                        ctypes.byref(a), ctypes.byref(b), ctypes.byref(n),
                                        _ptr(decoded) if decoded is not None else None))
        return a.value, b.value, int(n.value)

    def exchange_raw_bytes(self):
        """Bytes the exchanges since the last call would have moved uncoded; resets."""
        v = ctypes.c_int64()
        _check(lib().misort_exchange_raw_bytes(self._h, ctypes.byref(v)))
        return int(v.value)

    def exchange_stats(self):
        """(stages, bytes moved, bytes a whole-block exchange would move); resets."""
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(lib().misort_exchange_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    # ---- profiling ----------------------------------------------------------------
    def profile(self, on=True):
        _check(lib().misort_profile_enable(self._h, int(on)))

    def profile_reset(self):
        _check(lib().misort_profile_reset(self._h))

    def pass_probe(self, inp, out, kind, hi, r, flip, reps=5, n=None):
        """Average ms of one HBM pass of a plan shape (tile_sort, run_merge or run_mergek)."""
        ms = ctypes.c_float()
        k = KIND_NAMES.index(kind) if isinstance(kind, str) else int(kind)
        _check(lib().misort_pass_probe(self._h, _dtype_of(inp), _ptr(inp), _ptr(out),
                                       inp.numel() if n is None else n, k, hi, r, int(flip), reps,
                                       ctypes.byref(ms)))
        return ms.value

    def profile_stages(self, nstages):
        """Per hypercube stage: [(sorts, exchange_ms, merge_ms, exchange_bytes)]."""
        res = []
        for st in range(nstages):
            n, xm, mm, b = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            _check(lib().misort_profile_stage(self._h, st, ctypes.byref(n), ctypes.byref(xm),
                                              ctypes.byref(mm), ctypes.byref(b)))
            res.append((int(n.value), float(xm.value), float(mm.value), float(b.value)))
        return res

    def profile_trace(self):
        """[(kind_name, ms, algorithmic_bytes)] of every profiled record since the
        last reset, in completion order (a pass after the kernel nested in it)."""
        n = _check(lib().misort_profile_trace(self._h, 0, None, None, None))
        k = (ctypes.c_int32 * max(n, 1))()
        ms = (ctypes.c_double * max(n, 1))()
        b = (ctypes.c_double * max(n, 1))()
        _check(lib().misort_profile_trace(self._h, n, k, ms, b))
        return [(KIND_NAMES[k[i]], ms[i], b[i]) for i in range(n)]

    def profile_read(self):
        """{kind: (launches, total_ms, algorithmic_bytes)}."""
        res = {}
        for k, name in enumerate(KIND_NAMES):
            n, ms, b = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            _check(lib().misort_profile_read(self._h, k, ctypes.byref(n), ctypes.byref(ms),
                                             ctypes.byref(b)))
            res[name] = (int(n.value), float(ms.value), float(b.value))
        return res
