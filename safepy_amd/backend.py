"""Thin object layer over the C ABI: device context, device buffers and the three
device-resident handles (membership, attribute matrix, permutation tables).

Nothing here computes: every method forwards to libsafe_hip.so, and fails loudly if the
library reports an error (no HIP device, bad arguments, ...).
"""
import collections
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import lib, check

_SCORE = {'sum': _lib.SCORE_SUM, 'z-score': _lib.SCORE_ZSCORE}
_SIGN = {'highest': _lib.SIGN_HIGHEST, 'lowest': _lib.SIGN_LOWEST, 'both': _lib.SIGN_BOTH}


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _xy(xy, who, n=None):
    """Layout coordinates as the library reads them: C-contiguous f64 [n, 2] (any n when none is given)."""
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2 or (n is not None and xy.shape[0] != n):
        raise ValueError('%s: xy must be [%s, 2], got shape %s' % (who, 'n' if n is None else n, xy.shape))
    return xy


def _edges(edge_u, edge_v, edge_w, who):
    """An edge list as the library reads it: int32 end points and f64 weights (None = unit weights), one-dimensional, one length."""
    eu = np.ascontiguousarray(edge_u, dtype=np.int32)
    ev = np.ascontiguousarray(edge_v, dtype=np.int32)
    ew = None if edge_w is None else np.ascontiguousarray(edge_w, dtype=np.float64)
    if eu.shape != ev.shape or eu.ndim != 1 or (ew is not None and ew.shape != eu.shape):
        raise ValueError('%s: edge_u, edge_v (and edge_w) must be one-dimensional arrays of one length' % who)
    return eu, ev, ew


def _split_off_cores(cpus, n_cores, slot=0):
    """(CPUs of `n_cores` whole physical cores, the rest) of the CPU set `cpus`, or None when the topology cannot be read or
    fewer than n_cores + 2 cores would be left."""
    by_core = {}
    for c in sorted(cpus):
        try:
            sib = set()
            for part in open('/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list' % c).read().strip().split(','):
                lo, _, hi = part.partition('-')
                sib.update(range(int(lo), int(hi or lo) + 1))
        except OSError:
            return None
        if sib <= cpus:                                   # only cores whose hardware threads are all ours to use
            by_core[min(sib)] = sib
    cores = sorted(by_core)
    if len(cores) < n_cores * (slot + 1) + 2:
        return None
    taken = []                                            # core after core (the library gives each of its two draw threads one half)
    hi = len(cores) - n_cores * slot                      # (ranks of one node take different cores: slot = local rank)
    for c in cores[hi - n_cores:hi]:
        taken += sorted(by_core[c])
    return taken, set(cpus) - set(taken)


def pin_threads_to_device_numa(device=0, reserve_draw_cores=0):
    """Keep every thread this process has -- and those it starts later: the draw thread -- on the CPUs of the NUMA node the GPU hangs off.  A container may be scheduled on any CPU of a
    two-socket host; with the draw thread on the far socket a whole run is ~15-20 % slower (5.2 vs 5.4-6.2
    ms/step at configs[1]).  Returns the node, or None when the topology cannot be read (nothing is changed
    then).  For launchers (bench.py, run_batch): a library does not re-pin its caller behind its back.
    reserve_draw_cores = k > 0: k whole physical cores of that node are set aside for the library's draw thread
    (safe_set_draw_cpus) and every other thread of the process is kept off them."""
    import os
    try:
        buf = C.create_string_buffer(32)
        check(lib.safe_device_pci_bus_id(int(device), buf, 32))
        bdf = buf.value.decode().lower()
        node = int(open('/sys/bus/pci/devices/%s/numa_node' % bdf).read())
        if node < 0:
            return None
        cpus = set()
        for part in open('/sys/devices/system/node/node%d/cpulist' % node).read().strip().split(','):
            lo, _, hi = part.partition('-')
            cpus.update(range(int(lo), int(hi or lo) + 1))
        cpus &= os.sched_getaffinity(0)
        if not cpus:
            return None
        mine = cpus
        if reserve_draw_cores:
            # whole physical cores for the library's draw thread: nothing else of this process then shares a core with it
            # (a polling launcher on the sibling hardware thread slows the sequential draw chain by a third)
            split = _split_off_cores(cpus, int(reserve_draw_cores), int(device))
            if split is not None:
                draw_cpus, mine = split
                arr = (C.c_int * len(draw_cpus))(*draw_cpus)
                check(lib.safe_set_draw_cpus(arr, len(draw_cpus)))
        for tid in os.listdir('/proc/self/task'):
            try:
                os.sched_setaffinity(int(tid), mine)
            except OSError:
                pass
        return node
    except Exception:
        return None


class DeviceBuffer:
    """A raw device allocation owned by the library allocator (f64/i64 element views).  Freed buffers
    of 1 MiB and more go back to a per-context pool keyed by size: hipMalloc / hipFree of the result
    matrices (GBs at 20 000 nodes) cost tens of milliseconds per call, more than the kernels.
    The pool is bounded by a share of the device's memory (POOL_FRACTION of ctx.hbm_bytes); when a
    returned buffer does not fit, the sizes that have gone unused the longest are released first, and an
    allocation that fails returns the whole pool to the driver and tries once more."""

    POOL_FRACTION = 1.0 / 6.0             # of the device memory (48 GB of 288 GB)

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        pooled = ctx._pool.get(self.nbytes)
        if pooled:
            self.ptr = pooled.pop()
            ctx._pool_bytes -= self.nbytes
            if pooled:
                ctx._pool.move_to_end(self.nbytes)         # most recently used size last
            else:
                del ctx._pool[self.nbytes]
            return
        p = C.c_void_p()
        rc = lib.safe_dev_alloc(ctx.handle, max(self.nbytes, 1), C.byref(p))
        if rc != 0 and ctx._pool_bytes:                    # out of memory with buffers idling in the pool: release them, retry
            ctx.trim()
            rc = lib.safe_dev_alloc(ctx.handle, max(self.nbytes, 1), C.byref(p))
        check(rc)
        self.ptr = p.value

    def free(self):
        if self.ptr:
            ctx = self.ctx
            limit = int(ctx.hbm_bytes * self.POOL_FRACTION)
            if (1 << 20) <= self.nbytes <= limit:
                while ctx._pool and ctx._pool_bytes + self.nbytes > limit:     # evict the least recently used size
                    size, ptrs = next(iter(ctx._pool.items()))
                    check(lib.safe_dev_free(ctx.handle, C.c_void_p(ptrs.pop())))
                    ctx._pool_bytes -= size
                    if not ptrs:
                        del ctx._pool[size]
                ctx._pool.setdefault(self.nbytes, []).append(self.ptr)
                ctx._pool.move_to_end(self.nbytes)
                ctx._pool_bytes += self.nbytes
            else:
                check(lib.safe_dev_free(ctx.handle, C.c_void_p(self.ptr)))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def upload(self, host):
        host = np.ascontiguousarray(host)
        assert host.nbytes <= self.nbytes
        check(lib.safe_memcpy_h2d(self.ctx.handle, C.c_void_p(self.ptr), _ptr(host), host.nbytes))

    def download(self, shape, dtype=np.float64, out=None):
        """Copy to the host: into a fresh array, or into `out` (an array whose pages are resident -- it has been written
        before -- takes the plain copy at the link's rate; a fresh one the threaded copy that spreads its page faults)."""
        if out is not None:
            assert out.shape == tuple(shape) and out.dtype == dtype and out.flags.c_contiguous and out.nbytes <= self.nbytes
            check(lib.safe_memcpy_d2h_resident(self.ctx.handle, _ptr(out), C.c_void_p(self.ptr), out.nbytes))
            return out
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(lib.safe_memcpy_d2h(self.ctx.handle, _ptr(out), C.c_void_p(self.ptr), out.nbytes))
        return out

    def zero(self):
        check(lib.safe_dev_memset(self.ctx.handle, C.c_void_p(self.ptr), 0, self.nbytes))


class Context:
    _default = {}

    def __init__(self, device=0):
        h = C.c_void_p()
        check(lib.safe_ctx_create(int(device), C.byref(h)))
        self.handle = h
        self.device = int(device)
        ncu = C.c_int()
        hbm = C.c_int64()
        arch = C.create_string_buffer(64)
        check(lib.safe_ctx_info(h, C.byref(ncu), C.byref(hbm), arch, 64))
        self.num_cu = ncu.value
        self.hbm_bytes = hbm.value
        self.arch = arch.value.decode()
        self._pool = collections.OrderedDict()     # size -> [device pointers] of released DeviceBuffers, least recently used first
        self._pool_bytes = 0

    @classmethod
    def default(cls, device=0):
        """Process-wide context per device (created on first use)."""
        if device not in cls._default:
            cls._default[device] = cls(device)
        return cls._default[device]

    def set_stream(self, stream_ptr):
        check(lib.safe_ctx_set_stream(self.handle, C.c_void_p(stream_ptr) if stream_ptr else None))

    shared_stream = None        # (name, local_rank, local_world) once share_stream() has attached this context to a node's ring

    def share_stream(self, name, local_rank, local_world, capacity_bytes=64 << 20):
        """One permutation stream per node (safe_ctx_share_stream): local rank 0 draws, the other ranks of the node receive
        every chunk's row maps through a shared-memory ring.  Collective over the ranks of the node; afterwards
        Permutations(..., shared=True) on this context uses the ring."""
        if int(local_world) <= 1:
            return False
        check(lib.safe_ctx_share_stream(self.handle, str(name).encode(), int(local_rank), int(local_world), int(capacity_bytes)))
        self.shared_stream = (str(name), int(local_rank), int(local_world))
        return True

    def unshare_stream(self):
        check(lib.safe_ctx_unshare_stream(self.handle))
        self.shared_stream = None

    def sync(self):
        check(lib.safe_ctx_sync(self.handle))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def trim(self):
        """Return the pooled device buffers to the driver."""
        for ptrs in self._pool.values():
            for p in ptrs:
                check(lib.safe_dev_free(self.handle, C.c_void_p(p)))
        self._pool.clear()
        self._pool_bytes = 0

    def alloc_f64(self, *shape):
        return DeviceBuffer(self, int(np.prod(shape)) * 8)

    def timer_start(self):
        check(lib.safe_timer_start(self.handle))

    def timer_stop_ms(self):
        ms = C.c_double()
        check(lib.safe_timer_stop_ms(self.handle, C.byref(ms)))
        return ms.value

    def last_kernel(self):
        name = C.create_string_buffer(128)
        ms = C.c_double()
        cnt = C.c_int64()
        check(lib.safe_last_kernel_stats(self.handle, name, 128, C.byref(ms), C.byref(cnt)))
        return name.value.decode(), ms.value, cnt.value

    def last_rank_stats(self):
        """(k_rank_keys, k_rank_sort, k_rank_emit) times in ms of the context's last Attributes.rank()."""
        ms = [C.c_double() for _ in range(3)]
        check(lib.safe_last_rank_stats(self.handle, *[C.byref(x) for x in ms]))
        return tuple(x.value for x in ms)

    def last_diffusion_stats(self):
        """(ms of all k_diffusion_step launches, their number, ms of k_diffusion_transform) of the context's last Neighborhoods.diffusion()."""
        steps_ms, steps, transform_ms = C.c_double(), C.c_int(), C.c_double()
        check(lib.safe_last_diffusion_stats(self.handle, C.byref(steps_ms), C.byref(steps), C.byref(transform_ms)))
        return steps_ms.value, steps.value, transform_ms.value

    def last_kernel_busy_ms(self):
        """Time during which at least one launch of the dominant kernel of the last call was running (launches overlap)."""
        ms = C.c_double()
        check(lib.safe_last_kernel_busy_ms(self.handle, C.byref(ms)))
        return ms.value

    def edge_lengths(self, xy, edge_u, edge_v):
        xy = _xy(xy, 'edge_lengths')
        eu, ev, _ = _edges(edge_u, edge_v, None, 'edge_lengths')
        out = np.empty(eu.shape[0], dtype=np.float64)
        check(lib.safe_edge_lengths(self.handle, _ptr(xy), xy.shape[0], eu.shape[0], _ptr(eu), _ptr(ev), _ptr(out)))
        return out

    def pair_distance_select(self, xy, ranks):
        """Order statistics of scipy's pdist(xy) without the N (N - 1) / 2 distances (safe_pair_distance_select_xy): the
        elements of the 0-based `ranks` of the ascending multiset, bit for bit.  Returns (values f64 [len(ranks)], number
        of pairs); no ranks = the count alone."""
        xy = _xy(xy, 'pair_distance_select')
        rk = np.ascontiguousarray(np.atleast_1d(ranks), dtype=np.int64)
        out = np.empty(rk.shape[0], dtype=np.float64)
        count = C.c_int64(0)
        check(lib.safe_pair_distance_select_xy(self.handle, _ptr(xy), xy.shape[0], _ptr(rk) if rk.size else None, rk.shape[0],
                                               _ptr(out) if rk.size else None, C.byref(count)))
        return out, count.value

    def row_distance_select(self, xy, k):
        """Per node, the distance to its k-th nearest other node under scipy's pdist(xy), bit for bit
        (safe_row_distance_select_xy): f64 [n]; the farthest node where k exceeds n - 1, 0.0 for a single node."""
        xy = _xy(xy, 'row_distance_select')
        out = np.empty(xy.shape[0], dtype=np.float64)
        check(lib.safe_row_distance_select_xy(self.handle, _ptr(xy), xy.shape[0], int(k), _ptr(out)))
        return out

    def layout_spring(self, row_ptr, col, weight, pos0, k, iterations, threshold, dtype):
        """networkx's Fruchterman-Reingold iterations on the device (safe_layout_spring): CSR adjacency with
        strictly increasing columns per row (weight None = 1), pos0 [n,2] f64, dtype np.float32 (the sparse
        form networkx runs from 500 nodes) or np.float64.  Returns (positions [n,2] in dtype, iterations run)."""
        pos0 = np.ascontiguousarray(pos0, dtype=np.float64)
        n = pos0.shape[0]
        rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
        cl = np.ascontiguousarray(col, dtype=np.int32)
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
        if rp.shape[0] != n + 1 or cl.shape[0] != rp[-1] or (w is not None and w.shape[0] != cl.shape[0]):
            raise ValueError('layout_spring: CSR arrays do not match %d nodes' % n)
        # any other dtype goes to the library as a code it refuses (SafeHipError), like every other bad argument
        code = {np.dtype(np.float32): _lib.DTYPE_F32, np.dtype(np.float64): _lib.DTYPE_F64}.get(np.dtype(dtype), -1)
        out = np.empty((n, 2), dtype=np.float64)
        ran = C.c_int(0)
        check(lib.safe_layout_spring(self.handle, n, _ptr(rp), _ptr(cl) if cl.size else None,
                                     _ptr(w) if w is not None and w.size else None, code, _ptr(pos0), float(k),
                                     int(iterations), float(threshold), _ptr(out), C.byref(ran)))
        return out.astype(dtype), ran.value

    FORMAT_BUDGET = 64 << 20            # bytes of text per chunk of safe_format_tsv (two device and two pinned buffers of it)

    def format_tsv(self, values_dev_ptr, n, m, prefixes, prefix_offsets, fd, r0=0, r1=None, budget_bytes=None):
        """Rows [r0, r1) of the row-major [n, m] f64 device matrix at values_dev_ptr as pandas' to_csv(sep='\t') writes them,
        appended to the open file descriptor fd (safe_format_tsv): row r is prefixes[prefix_offsets[r - r0]:prefix_offsets[r - r0 + 1]]
        (bytes), '\t' + NumPy's text of each value (NaN: empty), '\n'.  Returns {'kernel_ms', 'copy_ms', 'write_ms', 'call_ms',
        'bytes'}."""
        r1 = n if r1 is None else r1
        pre = np.frombuffer(bytes(prefixes), dtype=np.uint8) if len(prefixes) else np.zeros(1, np.uint8)
        off = np.ascontiguousarray(prefix_offsets, dtype=np.int64)
        if off.shape != (r1 - r0 + 1,):
            raise ValueError('format_tsv: %d prefix offsets for %d rows' % (off.shape[0], r1 - r0))
        stats = (C.c_double * 5)()
        check(lib.safe_format_tsv(self.handle, C.c_void_p(values_dev_ptr) if values_dev_ptr else None, int(n), int(m), int(r0),
                                  int(r1), _ptr(pre), _ptr(off), int(fd), int(budget_bytes or self.FORMAT_BUDGET), stats))
        return dict(zip(('kernel_ms', 'copy_ms', 'write_ms', 'call_ms', 'bytes'), list(stats)))

    def _device_matrix(self, values, n, m):
        """(device pointer, temporary buffer or None) of a row-major [n, m] f64 matrix given as a device pointer (int, e.g. a
        _DeviceResult's buf.ptr; n and m required) or as a host array (uploaded into a temporary buffer)."""
        if isinstance(values, (int, np.integer)):
            if n is None or m is None:
                raise ValueError('a device pointer needs n and m')
            return int(values), None, int(n), int(m)
        host = np.ascontiguousarray(values, dtype=np.float64)
        if host.ndim != 2:
            raise ValueError('expected a [n, m] matrix, got shape %s' % (host.shape,))
        tmp = self.alloc_f64(*host.shape)
        tmp.upload(host)
        return tmp.ptr, tmp, host.shape[0], host.shape[1]

    def kde_grid(self, offsets, pts, weights, norm, xi):
        """SciPy's gaussian_kernel_estimate for D whitened 2-D point sets at once (safe_kde_grid): set d is pts[offsets[d]:
        offsets[d + 1]] (f64 [., 2]) with weights and norm[d], evaluated at xi[d] (f64 [D, G, 2]).  Returns (z [D, G], kernel
        ms)."""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        norm = np.ascontiguousarray(norm, dtype=np.float64).reshape(-1)
        xi = np.ascontiguousarray(xi, dtype=np.float64)
        d = off.shape[0] - 1
        if d < 0 or xi.ndim != 3 or xi.shape[0] != d or xi.shape[2] != 2 or norm.shape[0] != d:
            raise ValueError('kde_grid: %d offsets, xi %s, %d norms' % (off.shape[0], xi.shape, norm.shape[0]))
        if d and (off[-1] != pts.shape[0] or w.shape[0] != pts.shape[0]):
            raise ValueError('kde_grid: offsets end at %d for %d points and %d weights' % (off[-1], pts.shape[0], w.shape[0]))
        g = xi.shape[1]
        z = np.empty((d, g), dtype=np.float64)
        ms = C.c_double()
        check(lib.safe_kde_grid(self.handle, d, _ptr(off), _ptr(pts), _ptr(w), _ptr(norm), g, _ptr(xi), _ptr(z), C.byref(ms)))
        return z, ms.value

    def domain_counts(self, values, domain, n_domains, n=None, m=None):
        """f64 [n, n_domains]: the [n, m] matrix `values` (device pointer with n, m; or a host array) summed over the columns
        of each domain, domain int [m] in [0, n_domains) (safe_domain_counts).  Returns (counts, kernel ms)."""
        ptr, tmp, n, m = self._device_matrix(values, n, m)
        try:
            dom = np.ascontiguousarray(domain, dtype=np.int32)
            if dom.shape != (m,):
                raise ValueError('domain_counts: %d domain ids for %d columns' % (dom.size, m))
            out = np.empty((n, int(n_domains)), dtype=np.float64)
            ms = C.c_double()
            check(lib.safe_domain_counts(self.handle, C.c_void_p(ptr) if ptr else None, n, m, _ptr(dom), int(n_domains), _ptr(out),
                                         C.byref(ms)))
            return out, ms.value
        finally:
            if tmp is not None:
                tmp.free()

    def gather_columns(self, values, cols, n=None, m=None):
        """f64 [n, k]: columns `cols` of the [n, m] matrix `values` (device pointer with n, m; or a host array), copied without
        the rest of it (safe_gather_columns).  Returns (columns, kernel ms)."""
        ptr, tmp, n, m = self._device_matrix(values, n, m)
        try:
            cols = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1)
            out = np.empty((n, cols.shape[0]), dtype=np.float64)
            ms = C.c_double()
            check(lib.safe_gather_columns(self.handle, C.c_void_p(ptr) if ptr else None, n, m, _ptr(cols), cols.shape[0], _ptr(out),
                                          C.byref(ms)))
            return out, ms.value
        finally:
            if tmp is not None:
                tmp.free()

    NODE_DOMAINS_MAX = 2048             # domain ids safe_node_domains takes (two 8-byte LDS slots per id)

    def enriched_components_dev(self, values_dev_ptr, n, m, cols, edge_u, edge_v):
        """int32 [len(cols), n] component labels (smallest node id of the component; -1 = not enriched) of the columns `cols`
        of the row-major [n, m] f64 device matrix at values_dev_ptr, read in place (safe_enriched_components_dev): what
        enriched_components gives for the host slice values[:, cols].  Returns (labels, kernel ms)."""
        cols = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1)
        eu, ev, _ = _edges(edge_u, edge_v, None, 'enriched_components_dev')
        out = np.empty((cols.shape[0], int(n)), dtype=np.int32)
        ms = C.c_double()
        check(lib.safe_enriched_components_dev(self.handle, eu.shape[0], _ptr(eu) if eu.size else None, _ptr(ev) if ev.size else None,
                                               C.c_void_p(values_dev_ptr) if values_dev_ptr else None, int(n), int(m), _ptr(cols),
                                               cols.shape[0], _ptr(out), C.byref(ms)))
        return out, ms.value

    def enriched_pair_counts_dev(self, nbr, values_dev_ptr, n, m, cols):
        """(q, e, kernel ms) for the columns `cols` of the row-major [n, m] f64 device matrix at values_dev_ptr, read in place
        (safe_enriched_pair_counts_dev): int64 [len(cols)] each, e[a] = the number of nodes with value > 0 in column cols[a],
        q[a] = the sum of nbr's membership W[i, j] over the ordered pairs (i, j) of those nodes, the diagonal included -- what
        enriched_pair_counts gives for the host slice values[:, cols]."""
        cols = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1)
        q = np.empty(cols.shape[0], dtype=np.int64)
        e = np.empty(cols.shape[0], dtype=np.int64)
        ms = C.c_double()
        check(lib.safe_enriched_pair_counts_dev(self.handle, nbr.handle, C.c_void_p(values_dev_ptr) if values_dev_ptr else None, int(n),
                                                int(m), _ptr(cols), cols.shape[0], _ptr(q), _ptr(e), C.byref(ms)))
        return q, e, ms.value

    def profile_distances(self, values_dev_ptr, n, m, cols, metric):
        """scipy.spatial.distance.pdist(values[:, cols].T, metric), condensed, for the columns `cols` of the row-major [n, m]
        f64 device matrix at values_dev_ptr and a metric of _lib.METRIC_IDS (name or id), bit for bit (safe_profile_distances).
        Returns (distances f64 [k (k - 1) / 2], kernel ms)."""
        cols = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1)
        if isinstance(metric, str):
            if metric not in _lib.METRIC_IDS:
                raise ValueError('profile_distances: no kernel for metric %r (have: %s)' % (metric, ', '.join(_lib.METRIC_IDS)))
            metric = _lib.METRIC_IDS[metric]
        k = cols.shape[0]
        out = np.empty(k * (k - 1) // 2, dtype=np.float64)
        ms = C.c_double()
        check(lib.safe_profile_distances(self.handle, C.c_void_p(values_dev_ptr) if values_dev_ptr else None, int(n), int(m), _ptr(cols),
                                         k, int(metric), _ptr(out), C.byref(ms)))
        return out, ms.value

    LINKAGE_MAX_POINTS = _lib.LINKAGE_MAX_POINTS   # points the linkage kernel takes (8 n^2 bytes of working matrix, 16-bit chain ids)

    def linkage_average(self, cond, m_top=None):
        """scipy.cluster.hierarchy.linkage(cond, method='average'), bit for bit (safe_linkage_average): cond is the condensed
        f64 distance vector of m_top points, as a device pointer (int; m_top required; read on the context's stream, not
        modified) or as a host array that is uploaded.  Distances that are not all finite raise SafeHipError with code
        E_VALUE, more than LINKAGE_MAX_POINTS points E_UNSUPPORTED.  Returns (Z f64 [m_top - 1, 4], kernel ms)."""
        tmp = None
        if isinstance(cond, (int, np.integer)):
            if m_top is None:
                raise ValueError('linkage_average: a device pointer needs m_top')
            ptr, k = int(cond), int(m_top)
        else:
            host = np.ascontiguousarray(cond, dtype=np.float64).reshape(-1)
            k = int(round((1 + np.sqrt(1 + 8 * host.shape[0])) / 2)) if m_top is None else int(m_top)
            if k * (k - 1) // 2 != host.shape[0]:
                raise ValueError('linkage_average: %d distances are not the condensed form of %d points' % (host.shape[0], k))
            ptr = 0
            if 2 <= k <= self.LINKAGE_MAX_POINTS:                        # (the library refuses the other sizes before it reads)
                tmp = self.alloc_f64(host.shape[0])
                tmp.upload(host)
                ptr = tmp.ptr
        try:
            z = np.empty((max(k - 1, 0), 4), dtype=np.float64)
            ms = C.c_double()
            check(lib.safe_linkage_average(self.handle, C.c_void_p(ptr) if ptr else None, k, _ptr(z), C.byref(ms)))
            return z, ms.value
        finally:
            if tmp is not None:
                tmp.free()

    def profile_linkage(self, values_dev_ptr, n, m, cols, metric):
        """linkage(pdist(values[:, cols].T, metric), method='average') of SciPy for the columns `cols` of the row-major [n, m]
        f64 device matrix at values_dev_ptr and a metric of _lib.METRIC_IDS (name or id): the kernels of profile_distances,
        then linkage_average's, without the condensed vector leaving the device (safe_profile_linkage).  Raises like
        linkage_average.  Returns (Z f64 [k - 1, 4], kernel ms)."""
        cols = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1)
        if isinstance(metric, str):
            if metric not in _lib.METRIC_IDS:
                raise ValueError('profile_linkage: no kernel for metric %r (have: %s)' % (metric, ', '.join(_lib.METRIC_IDS)))
            metric = _lib.METRIC_IDS[metric]
        k = cols.shape[0]
        z = np.empty((max(k - 1, 0), 4), dtype=np.float64)
        ms = C.c_double()
        check(lib.safe_profile_linkage(self.handle, C.c_void_p(values_dev_ptr) if values_dev_ptr else None, int(n), int(m), _ptr(cols),
                                       k, int(metric), _ptr(z), C.byref(ms)))
        return z, ms.value

    def node_domains(self, nes_binary_dev_ptr, nes_dev_ptr, n, m, domain, ids):
        """define_domains' node table from the two row-major [n, m] f64 device matrices, one pass (safe_node_domains): domain
        int [m] is every attribute's domain id, ids the sorted distinct ids.  Returns (sums f64 [n, len(ids)], primary int32
        [n], primary_nes f64 [n], kernel ms)."""
        dom = np.ascontiguousarray(domain, dtype=np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        if dom.shape != (int(m),):
            raise ValueError('node_domains: %d domain ids for %d columns' % (dom.size, m))
        sums = np.empty((int(n), ids.shape[0]), dtype=np.float64)
        primary = np.empty(int(n), dtype=np.int32)
        pnes = np.empty(int(n), dtype=np.float64)
        ms = C.c_double()
        check(lib.safe_node_domains(self.handle, C.c_void_p(nes_binary_dev_ptr) if nes_binary_dev_ptr else None,
                                    C.c_void_p(nes_dev_ptr) if nes_dev_ptr else None, int(n), int(m), _ptr(dom), _ptr(ids), ids.shape[0],
                                    _ptr(sums), _ptr(primary), _ptr(pnes), C.byref(ms)))
        return sums, primary, pnes, ms.value

    def enriched_pairs(self, selector_ptr, values_ptr, n, m, mode, threshold, axis):
        """The selected cells of the row-major [n, m] f64 device matrix at selector_ptr as the arrays of a scipy.sparse CSR
        (axis 0) or CSC (axis 1) matrix, compacted on the device (safe_pairs_create / _read / _destroy; modes: Pairs.MODES).
        values_ptr: the [n, m] device matrix whose cells become `data` (may be selector_ptr), or None for the pattern alone
        (data is then None).  Neither matrix is written, freed or copied whole.  Returns (indptr int32 [n + 1] or [m + 1],
        indices int32 [nnz], data f64 [nnz] or None, (count kernels ms, emit kernel ms))."""
        pairs = Pairs(self, selector_ptr, n, m, mode, threshold, axis)
        try:
            indptr, indices, data, read_ms = pairs.read(selector_ptr, values_ptr)
            return indptr, indices, data, (pairs.create_ms, read_ms)
        finally:
            pairs.close()

    def euclidean_dense(self, xy_dev_ptr, n, nr, mask_dev_ptr=None, dist_dev_ptr=None):
        check(lib.safe_euclidean_dense_dev(self.handle, C.c_void_p(xy_dev_ptr), int(n), float(nr),
                                           C.c_void_p(mask_dev_ptr) if mask_dev_ptr else None,
                                           C.c_void_p(dist_dev_ptr) if dist_dev_ptr else None))


class Neighborhoods:
    """Device-resident membership (bit matrix + CSR + SELL-64)."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.handle = handle
        n, nnz, mx = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib.safe_nbr_info(handle, C.byref(n), C.byref(nnz), C.byref(mx)))
        self.n, self.nnz, self.max_row_count = n.value, nnz.value, mx.value
        self.has_weights = False         # set_weights* / clear_weights

    @classmethod
    def euclidean(cls, ctx, xy, nr):
        xy = _xy(xy, 'euclidean')
        h = C.c_void_p()
        check(lib.safe_nbr_euclidean(ctx.handle, _ptr(xy), xy.shape[0], float(nr), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def shortpath(cls, ctx, n, edge_u, edge_v, edge_w, cutoff, keep_distances=False):
        eu, ev, ew = _edges(edge_u, edge_v, edge_w, 'shortpath')
        h = C.c_void_p()
        check(lib.safe_nbr_shortpath(ctx.handle, int(n), eu.shape[0], _ptr(eu), _ptr(ev), _ptr(ew), float(cutoff),
                                     1 if keep_distances else 0, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def diffusion(cls, ctx, n, edge_u, edge_v, edge_w, restart, steps, cutoff, want_kernel=False):
        """The random-walk-with-restart handle (safe_nbr_diffusion): A[i, j] = (D[i, j] <= cutoff and reached), the distances
        kept as a shortest-path handle keeps them.  edge_w: None = unit weights.  want_kernel: returns (handle, K f64 [n, n])."""
        eu, ev, ew = _edges(edge_u, edge_v, edge_w, 'diffusion')
        kernel = np.empty((int(n), int(n)), dtype=np.float64) if want_kernel else None
        h = C.c_void_p()
        check(lib.safe_nbr_diffusion(ctx.handle, int(n), eu.shape[0], _ptr(eu), _ptr(ev), _ptr(ew), float(restart), int(steps),
                                     float(cutoff), _ptr(kernel), C.byref(h)))
        nbr = cls(ctx, h)
        return (nbr, kernel) if want_kernel else nbr

    @classmethod
    def from_dense(cls, ctx, a):
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError('neighborhoods must be a square matrix, got shape %s' % (a.shape,))
        a = np.ascontiguousarray(a, dtype=np.int64)
        h = C.c_void_p()
        check(lib.safe_nbr_from_dense_i64(ctx.handle, _ptr(a), a.shape[0], C.byref(h)))
        return cls(ctx, h)

    @staticmethod
    def _radii(radii, n, who):
        r = np.ascontiguousarray(radii, dtype=np.float64)
        if r.shape != (n,):
            raise ValueError('%s: radii must be one number per node, shape (%d,), got %s' % (who, n, r.shape))
        return r

    @classmethod
    def euclidean_rows(cls, ctx, xy, radii):
        """A[i, j] = (pdist distance of i and j <= radii[i]): one radius per row (safe_nbr_euclidean_rows)."""
        xy = _xy(xy, 'euclidean_rows')
        r = cls._radii(radii, xy.shape[0], 'euclidean_rows')
        h = C.c_void_p()
        check(lib.safe_nbr_euclidean_rows(ctx.handle, _ptr(xy), xy.shape[0], _ptr(r), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_distances_rows(cls, src, radii, keep_distances=False):
        """A new handle of A[i, j] = (D[i, j] <= radii[i]) over the reached pairs of the matrix D that `src` kept
        (safe_nbr_from_distances_rows); `src` is not changed.  keep_distances: the new handle keeps D where A is 1, +inf elsewhere."""
        r = cls._radii(radii, src.n, 'from_distances_rows')
        h = C.c_void_p()
        check(lib.safe_nbr_from_distances_rows(src.handle, _ptr(r), 1 if keep_distances else 0, C.byref(h)))
        return cls(src.ctx, h)

    def row_distance_select(self, k):
        """Per node, the k-th smallest finite kept distance to another node (safe_nbr_row_distance_select): f64 [n]; the
        farthest reached node where k exceeds their number, 0.0 for a node that reaches no other."""
        out = np.empty(self.n, dtype=np.float64)
        check(lib.safe_nbr_row_distance_select(self.handle, int(k), _ptr(out)))
        return out

    def set_layout(self, xy):
        """Hint: the 2-D layout the membership came from (node order of the matrix-core kernel only)."""
        xy = _xy(xy, 'set_layout', self.n)
        check(lib.safe_nbr_set_layout(self.handle, _ptr(xy)))

    def to_dense(self):
        out = np.empty((self.n, self.n), dtype=np.int64)
        check(lib.safe_nbr_to_dense_i64(self.handle, _ptr(out)))
        return out

    def to_dense_dev(self, dev_ptr):
        check(lib.safe_nbr_to_dense_i64_dev(self.handle, C.c_void_p(dev_ptr)))

    def row_counts(self):
        out = np.empty(self.n, dtype=np.int64)
        check(lib.safe_nbr_row_counts(self.handle, _ptr(out)))
        return out

    def csr(self):
        rp = np.empty(self.n + 1, dtype=np.int32)
        col = np.empty(max(self.nnz, 1), dtype=np.int32)
        check(lib.safe_nbr_csr(self.handle, _ptr(rp), _ptr(col)))
        return rp, col[:self.nnz]

    def distances(self):
        out = np.empty((self.n, self.n), dtype=np.float64)
        check(lib.safe_nbr_distances(self.handle, _ptr(out)))
        return out

    def distance_select(self, ranks):
        """Order statistics of the kept distances D[i, j], i < j, finite (safe_nbr_distance_select), read on the device:
        (values f64 [len(ranks)], number of finite pairs); no ranks = the count alone."""
        rk = np.ascontiguousarray(np.atleast_1d(ranks), dtype=np.int64)
        out = np.empty(rk.shape[0], dtype=np.float64)
        count = C.c_int64(0)
        check(lib.safe_nbr_distance_select(self.handle, _ptr(rk) if rk.size else None, rk.shape[0],
                                           _ptr(out) if rk.size else None, C.byref(count)))
        return out, count.value

    # ---- distance weights: one f64 per member, in the order of csr() (weights.hip) ----
    @staticmethod
    def _weight_kind(kind):
        if kind not in _lib.WEIGHT_KINDS:
            raise ValueError('%r is not a weight kind. Valid options are: %s' % (kind, ', '.join(_lib.WEIGHT_KINDS)))
        return _lib.WEIGHT_KINDS[kind]

    def set_weights_from_xy(self, xy, kind, radii, bandwidth=0.5):
        """Weights of every member from the pdist distance of the coordinates and the row's radius
        (safe_nbr_weights_from_xy); kind: 'uniform', 'triangular', 'epanechnikov', 'gaussian'; radii: a number or one per node."""
        xy = _xy(xy, 'set_weights_from_xy', self.n)
        r = self._radii(np.broadcast_to(np.asarray(radii, dtype=np.float64), (self.n,)), self.n, 'set_weights_from_xy')
        check(lib.safe_nbr_weights_from_xy(self.handle, _ptr(xy), self._weight_kind(kind), _ptr(r), float(bandwidth)))
        self.has_weights = True

    def set_weights_from_distances(self, kind, radii, bandwidth=0.5):
        """The same from the distance matrix the handle kept (safe_nbr_weights_from_distances)."""
        r = self._radii(np.broadcast_to(np.asarray(radii, dtype=np.float64), (self.n,)), self.n, 'set_weights_from_distances')
        check(lib.safe_nbr_weights_from_distances(self.handle, self._weight_kind(kind), _ptr(r), float(bandwidth)))
        self.has_weights = True

    def set_weights(self, w):
        """The caller's weights, f64 [nnz] in the order of csr(), finite and >= 0 (safe_nbr_set_weights)."""
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape != (self.nnz,):
            raise ValueError('set_weights: one weight per member, shape (%d,), got %s' % (self.nnz, w.shape))
        check(lib.safe_nbr_set_weights(self.handle, _ptr(w)))
        self.has_weights = True

    def weights(self):
        """f64 [nnz] in the order of csr() (safe_nbr_weights); SafeHipError when the handle has none."""
        out = np.empty(max(self.nnz, 1), dtype=np.float64)
        check(lib.safe_nbr_weights(self.handle, _ptr(out)))
        return out[:self.nnz]

    def clear_weights(self):
        check(lib.safe_nbr_clear_weights(self.handle))
        self.has_weights = False

    def close(self):
        if self.handle:
            check(lib.safe_nbr_destroy(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KamadaKawai:
    """networkx's Kamada-Kawai cost function for one matrix of preferred distances, device resident (safe_kk_*): what
    _kamada_kawai_solve prepares once -- 1 / (dist_mtx + eye * 1e-3) and its transpose, 16 n^2 bytes -- behind
    `evaluate`, the _kamada_kawai_costfn a minimiser calls."""

    MAX_NODES = _lib.KK_MAX_NODES

    def __init__(self, ctx, handle, n):
        self.ctx = ctx
        self.handle = handle
        self.n = int(n)
        self.evaluations = 0

    @classmethod
    def from_distances(cls, ctx, dist):
        """dist: [n, n] f64, dist[i][j] = preferred distance from node i to node j (inf counts as networkx's 1e6)."""
        d = np.ascontiguousarray(dist, dtype=np.float64)
        if d.ndim != 2 or d.shape[0] != d.shape[1] or d.shape[0] < 1:
            raise ValueError('the distance matrix must be square, got shape %s' % (d.shape,))
        h = C.c_void_p()
        check(lib.safe_kk_create_host(ctx.handle, _ptr(d), d.shape[0], C.byref(h)))
        return cls(ctx, h, d.shape[0])

    @classmethod
    def from_neighborhoods(cls, ctx, nbr):
        """From the all-pairs distances a Neighborhoods.shortpath(..., cutoff=inf, keep_distances=True) handle kept: they stay
        on the device."""
        h = C.c_void_p()
        check(lib.safe_kk_create_nbr(ctx.handle, nbr.handle, C.byref(h)))
        return cls(ctx, h, nbr.n)

    def evaluate(self, pos):
        """(cost, gradient [2n]) at the positions pos ([n, 2] or flat [2n]), as _kamada_kawai_costfn returns them."""
        x = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1)
        if x.shape[0] != 2 * self.n:
            raise ValueError('evaluate: expected %d coordinates, got %d' % (2 * self.n, x.shape[0]))
        grad = np.empty(2 * self.n, dtype=np.float64)
        cost = C.c_double()
        check(lib.safe_kk_eval(self.handle, _ptr(x), C.byref(cost), _ptr(grad)))
        self.evaluations += 1
        return np.float64(cost.value), grad

    def close(self):
        if self.handle:
            check(lib.safe_kk_destroy(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pairs:
    """One selection of a device-resident [n, m] f64 matrix, counted and scanned on the device (safe_pairs_create): `nnz`
    is known, `read` emits the indices and gathers values.  mode: 0 x > 0, 1 |x| > threshold, 2 x > threshold,
    3 x < -threshold (strict; NaN never); axis 0 by row (CSR), 1 by column (CSC).  Raises SafeHipError: E_INVALID for a bad
    mode or axis, E_VALUE for a NaN or negative threshold, E_UNSUPPORTED when a side or nnz reaches 2**31."""

    MODES = {'positive_nonzero': 0, 'both': 1, 'positive': 2, 'negative': 3}

    def __init__(self, ctx, selector_ptr, n, m, mode, threshold, axis):
        self.ctx = ctx
        self.handle = None
        self.n, self.m, self.axis = int(n), int(m), int(axis)
        h = C.c_void_p()
        nnz = C.c_int64()
        ms = C.c_double()
        check(lib.safe_pairs_create(ctx.handle, C.c_void_p(selector_ptr) if selector_ptr else None, self.n, self.m, int(mode),
                                    float(threshold), self.axis, C.byref(h), C.byref(nnz), C.byref(ms)))
        self.handle = h
        self.nnz = nnz.value
        self.create_ms = ms.value

    def read(self, selector_ptr, values_ptr=None, out=None):
        """(indptr, indices, data or None, emit kernel ms).  selector_ptr must hold what the constructor saw: SafeHipError
        E_VALUE otherwise, and nothing is written.  out: (indptr, indices, data) arrays to fill instead of fresh ones."""
        dim = self.n if self.axis == 0 else self.m
        if out is None:
            out = (np.empty(dim + 1, dtype=np.int32), np.empty(self.nnz, dtype=np.int32),
                   np.empty(self.nnz, dtype=np.float64) if values_ptr else None)
        indptr, indices, data = out
        if (indptr.shape, indptr.dtype) != ((dim + 1,), np.int32) or (indices.shape, indices.dtype) != ((self.nnz,), np.int32) or (
                values_ptr and (data.shape, data.dtype) != ((self.nnz,), np.float64)):
            raise ValueError('Pairs.read: output arrays of the wrong shape or type')
        ms = C.c_double()
        check(lib.safe_pairs_read(self.handle, C.c_void_p(selector_ptr) if selector_ptr else None,
                                  C.c_void_p(values_ptr) if values_ptr else None, _ptr(indptr), _ptr(indices),
                                  _ptr(data) if values_ptr else None, C.byref(ms)))
        return indptr, indices, data if values_ptr else None, ms.value

    def close(self):
        if self.handle:
            check(lib.safe_pairs_destroy(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GoClosure:
    """Direct (locus, term) annotations propagated to every ancestor term of an is_a DAG, on the device (safe_go_create): the
    CSC of the 0/1 [n_rows, n_kept] matrix stays there; `read` copies it out, `as_attributes` expands it into a device
    matrix.  child_ptr / child_idx: the children of every term (CSR, int32); ann_row / ann_term: the direct annotations
    (duplicates allowed); root: the term that takes the loci without one; missing_rows: loci the annotations do not know.
    Raises SafeHipError E_VALUE for a cycle, an index out of range or an annotation on a missing row."""

    PASSES = ('scatter', 'closure', 'count', 'root', 'scan', 'emit')

    def __init__(self, ctx, n_rows, n_terms, child_ptr, child_idx, ann_row, ann_term, root, missing_rows=None):
        self.ctx = ctx
        self.handle = None
        self.n_rows, self.n_terms = int(n_rows), int(n_terms)
        child_ptr = np.ascontiguousarray(child_ptr, dtype=np.int32)
        child_idx = np.ascontiguousarray(child_idx, dtype=np.int32)
        ann_row = np.ascontiguousarray(ann_row, dtype=np.int32)
        ann_term = np.ascontiguousarray(ann_term, dtype=np.int32)
        if child_ptr.shape != (self.n_terms + 1,) or ann_row.shape != ann_term.shape or ann_row.ndim != 1 or child_idx.ndim != 1:
            raise ValueError('GoClosure: child_ptr must hold n_terms + 1 offsets, ann_row and ann_term the same number of pairs')
        if child_idx.shape[0] < (int(child_ptr[-1]) if child_ptr.size else 0):
            raise ValueError('GoClosure: child_idx is shorter than child_ptr[-1]')
        mis = None
        if missing_rows is not None:
            mis = np.ascontiguousarray(np.asarray(missing_rows) != 0, dtype=np.uint8)
            if mis.shape != (self.n_rows,):
                raise ValueError('missing_rows: expected %d flags, got shape %s' % (self.n_rows, mis.shape))
        h = C.c_void_p()
        n_kept, nnz, assigned = C.c_int64(), C.c_int64(), C.c_int64()
        ms = C.c_double()
        check(lib.safe_go_create(ctx.handle, self.n_rows, self.n_terms, _ptr(child_ptr), _ptr(child_idx) if child_idx.size else None,
                                 ann_row.shape[0], _ptr(ann_row) if ann_row.size else None, _ptr(ann_term) if ann_term.size else None,
                                 int(root), _ptr(mis), C.byref(h), C.byref(n_kept), C.byref(nnz), C.byref(assigned), C.byref(ms)))
        self.handle = h
        self.n_kept, self.nnz, self.num_root_assigned = n_kept.value, nnz.value, assigned.value
        self.kernel_ms = ms.value

    def read(self):
        """(indptr int64 [n_kept + 1], indices int32 [nnz], kept int32 [n_kept], num_root_assigned)."""
        indptr = np.empty(self.n_kept + 1, dtype=np.int64)
        indices = np.empty(self.nnz, dtype=np.int32)
        kept = np.empty(self.n_kept, dtype=np.int32)
        assigned = C.c_int64()
        check(lib.safe_go_read(self.handle, _ptr(indptr), _ptr(indices) if self.nnz else None, _ptr(kept) if self.n_kept else None,
                               C.byref(assigned)))
        return indptr, indices, kept, assigned.value

    def as_attributes(self):
        """The f32 [n_rows, n_kept] matrix as a device handle (NaN across the missing rows), expanded where the CSC lies."""
        h = C.c_void_p()
        check(lib.safe_go_as_attr(self.handle, C.byref(h)))
        return Attributes(self.ctx, h, self.n_rows, self.n_kept, dtype=np.float32)

    def pass_ms(self):
        """({pass: ms of the create call}, number of levels)."""
        ms = (C.c_double * len(self.PASSES))()
        levels = C.c_int64()
        check(lib.safe_go_pass_ms(self.handle, ms, C.byref(levels)))
        return dict(zip(self.PASSES, list(ms))), levels.value

    def close(self):
        if self.handle:
            check(lib.safe_go_destroy(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _is_sparse(a):
    """scipy.sparse.issparse without importing SciPy for callers that never touch it."""
    import sys
    sp = sys.modules.get('scipy.sparse')
    if sp is None:
        if not type(a).__module__.startswith('scipy.sparse'):
            return False
        import scipy.sparse as sp
    return sp.issparse(a)


class Attributes:
    """Device-resident node x attribute matrix (f32/f64, C or Fortran order, NaN = missing)."""

    def __init__(self, ctx, handle, n, m, keepalive=None, dtype=None):
        self.ctx = ctx
        self.handle = handle
        self.n, self.m = n, m
        self._keepalive = keepalive
        self.dtype = None if dtype is None else np.dtype(dtype)      # of the device matrix, where the constructor knows it

    @staticmethod
    def _layout(b, allow_u8=False):
        if b.ndim != 2:
            raise ValueError('node2attribute must be 2-D, got shape %s' % (b.shape,))
        if b.dtype == np.float32:
            dt = _lib.DTYPE_F32
        elif b.dtype == np.float64:
            dt = _lib.DTYPE_F64
        elif allow_u8 and b.dtype in (np.uint8, np.bool_):
            # additive: a 0/1 matrix as bytes travels as bytes (a quarter of the f32 upload) and is f32 on the device
            b = b.view(np.uint8)
            dt = _lib.DTYPE_U8
        else:
            b = b.astype(np.float64)
            dt = _lib.DTYPE_F64
        if not (b.flags['C_CONTIGUOUS'] or b.flags['F_CONTIGUOUS']):
            b = np.ascontiguousarray(b)
        n, m = b.shape
        if b.flags['C_CONTIGUOUS']:
            rs, cs = m, 1
        else:
            rs, cs = 1, n
        return b, dt, n, m, rs, cs

    @staticmethod
    def canonical_csc(a):
        """Host side of from_sparse: any scipy.sparse matrix or array as (n, m, indptr int64 [m+1], indices int32 [nnz],
        values or None, owner), the input form of safe_attr_create_csc_host -- CSC with duplicates summed and row indices sorted,
        made on a copy this call owns unless the input is in that form already (`owner` keeps the arrays alive; the input is
        never modified).  values is None when every stored value is 1 (the
        library then makes an f32 matrix); f32 / f64 data otherwise stays as it is and bool / integer data becomes f64."""
        import scipy.sparse as sp
        if not sp.issparse(a):
            raise TypeError('canonical_csc: expected a scipy.sparse matrix or array, got %s' % type(a).__name__)
        if a.ndim != 2:
            raise ValueError('node2attribute must be 2-D, got shape %s' % (a.shape,))
        if a.format == 'csc' and a.has_canonical_format:
            c = a                                         # nothing to change, so nothing to copy (16 MB at 2 M stored entries)
        else:
            c = a.tocsc(copy=True)
            c.sum_duplicates()
            c.sort_indices()
        if c.dtype not in (np.float32, np.float64):
            c = c.astype(np.float64)                      # (after the conversion: duplicates meet in the input's own dtype, as in toarray())
        n, m = c.shape
        if c.nnz >= 1 << 31 or n >= 1 << 31:
            raise ValueError('sparse node2attribute: %d stored entries / %d rows do not fit 32-bit row indices' % (c.nnz, n))
        indptr = np.ascontiguousarray(c.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(c.indices, dtype=np.int32)
        values = np.ascontiguousarray(c.data)
        if bool((values == 1).all()):
            values = None
        return n, m, indptr, indices, values, c

    @classmethod
    def from_sparse(cls, ctx, a, missing_rows=None):
        """A scipy.sparse node x attribute matrix (any format) expanded on the device (safe_attr_create_csc_host): only the
        stored entries travel.  The handle equals from_host of the dense equivalent -- 0 where nothing is stored, stored
        zeros and NaNs kept, and NaN across every row i with missing_rows[i] != 0 (the nodes without a row in the file)."""
        n, m, indptr, indices, values, _keep = cls.canonical_csc(a)
        mis = None
        if missing_rows is not None:
            mis = np.ascontiguousarray(np.asarray(missing_rows) != 0, dtype=np.uint8)
            if mis.shape != (n,):
                raise ValueError('missing_rows: expected %d flags, got shape %s' % (n, mis.shape))
        dt = _lib.DTYPE_F64 if values is not None and values.dtype == np.float64 else _lib.DTYPE_F32
        h = C.c_void_p()
        check(lib.safe_attr_create_csc_host(ctx.handle, n, m, indices.shape[0], _ptr(indptr), _ptr(indices) if indices.size else None,
                                            _ptr(values), dt, _ptr(mis), C.byref(h)))
        return cls(ctx, h, n, m, dtype=np.float64 if dt == _lib.DTYPE_F64 else np.float32)

    @classmethod
    def from_host(cls, ctx, b):
        if _is_sparse(b):
            return cls.from_sparse(ctx, b)
        b, dt, n, m, rs, cs = cls._layout(np.asarray(b), allow_u8=True)
        h = C.c_void_p()
        check(lib.safe_attr_create_host(ctx.handle, _ptr(b), dt, n, m, rs, cs, C.byref(h)))
        return cls(ctx, h, n, m)

    @classmethod
    def from_device(cls, ctx, dev_ptr, dtype, n, m, order='C', keepalive=None):
        dt = _lib.DTYPE_F32 if np.dtype(dtype) == np.float32 else _lib.DTYPE_F64
        rs, cs = (m, 1) if order == 'C' else (1, n)
        h = C.c_void_p()
        check(lib.safe_attr_create_dev(ctx.handle, C.c_void_p(dev_ptr), dt, n, m, rs, cs, C.byref(h)))
        return cls(ctx, h, n, m, keepalive=keepalive)

    @classmethod
    def reindexed(cls, ctx, table, row_map, fill_value=np.nan, order='F', want_host=True):
        """read_attributes' alignment step (safe_io.py:386-390, 410): rows of the file's `table`
        gathered into node order on the device.  row_map[i] = table row of node i, -1 = absent
        (fill_value), -2 = masked duplicate (NaN).  Returns (handle, host copy or None); the host
        copy has the table's dtype and the requested memory order."""
        table, dt, nl, m, rs, cs = cls._layout(np.asarray(table))
        row_map = np.ascontiguousarray(row_map, dtype=np.int64)
        n = row_map.shape[0]
        host = np.empty((n, m), dtype=table.dtype, order=order) if want_host else None
        h = C.c_void_p()
        check(lib.safe_attr_reindex(ctx.handle, _ptr(table), dt, nl, m, rs, cs, _ptr(row_map), n, float(fill_value),
                                    0 if order == 'C' else 1, _ptr(host) if want_host else None, C.byref(h)))
        return cls(ctx, h, n, m), host

    def value_counts(self):
        """(#NaN, #zeros, #positives, #negatives) -- the census of safe_io.py:426-429."""
        v = [C.c_int64() for _ in range(4)]
        check(lib.safe_attr_value_counts(self.handle, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def nan_to_zero(self):
        """background='network' on the device copy (safe.py:449-451)."""
        check(lib.safe_attr_nan_to_zero(self.handle))

    def download(self, dtype, order='C'):
        out = np.empty((self.n, self.m), dtype=dtype, order=order)
        check(lib.safe_attr_download(self.handle, _ptr(out)))
        return out

    def stats(self):
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(lib.safe_attr_stats(self.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {'n_other': a.value, 'max_nan_col': b.value, 'n_rows_with_value': c.value, 'n_non_integer': d.value}

    def row_flags(self):
        out = np.empty(self.n, dtype=np.uint8)
        check(lib.safe_attr_row_flags(self.handle, _ptr(out)))
        return out

    def column_sums(self):
        """nansum of every column, f64 [m], as the statistics pass left it on the device (exact for integer-valued data)."""
        out = np.empty(self.m, dtype=np.float64)
        check(lib.safe_attr_column_sums(self.handle, _ptr(out)))
        return out

    def column_moments(self, col0=0, col1=None):
        """(mean, css) of columns [col0, col1), f64 each: the column's mean over the rows that hold a value (NaN cells inside
        them count as 0) and its centred sum of squares over the same rows, exactly 0 for a constant column
        (safe_attr_column_moments).  Two calls return the same bits."""
        col1 = self.m if col1 is None else col1
        mean, css = np.empty(max(col1 - col0, 0), dtype=np.float64), np.empty(max(col1 - col0, 0), dtype=np.float64)
        check(lib.safe_attr_column_moments(self.handle, int(col0), int(col1), _ptr(mean), _ptr(css)))
        return mean, css

    def set_row_flags(self, flags):
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        assert flags.shape == (self.n,)
        check(lib.safe_attr_set_row_flags(self.handle, _ptr(flags)))

    def rank(self):
        """A new handle that owns R, f64 [n, m] in Fortran order (read it with download(np.float64, order='F')): every column
        of this matrix replaced by its midranks among the column's non-NaN values, NaN where this matrix is NaN --
        scipy.stats.rankdata(b, method='average', axis=0, nan_policy='omit'), bit for bit, sorted on the device
        (safe_attr_rank).  This handle is not modified; the new one inherits its row flags, owns its memory (it keeps nothing
        of this handle alive) and is closed by the caller."""
        h = C.c_void_p()
        check(lib.safe_attr_rank(self.handle, C.byref(h)))
        return type(self)(self.ctx, h, self.n, self.m, dtype=np.float64)

    def close(self):
        if self.handle:
            check(lib.safe_attr_destroy(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


AttributeMatrix = Attributes        # the handle under the name of what it holds


class Permutations:
    """Device-resident composed row-permutation tables (legacy NumPy MT19937 stream)."""

    def __init__(self, ctx, n, movable, num_permutations, seed, shared=False, device_key=None):
        """seed: the reference's random_seed -- an integer reproduces np.random.seed(seed) + np.random.permutation exactly
        (safe_extras.py:46-58).  seed=None (the reference's default: OS entropy, nothing to reproduce) generates the tables
        ON THE DEVICE (safe_perms_create_device: i.i.d. uniform permutations, counter-based generator) keyed by `device_key`
        (64 bits; default: OS entropy) -- unless SAFE_HIP_DEVICE_STREAM=0 or more than 65535 rows move, then the NumPy-compatible
        stream runs from an entropy seed as before.
        shared=True: a COLLECTIVE call over the ranks of this node whose contexts share a stream (Context.share_stream):
        only the node's local rank 0 draws (its seed counts), the others receive the row maps.  Without a shared stream on
        the context it is the plain per-process stream.  (Device-generated tables need no sharing: every rank generates the
        same tables from the same key.)"""
        movable = np.ascontiguousarray(movable, dtype=np.uint8)
        assert movable.shape == (n,)
        if seed is not None:
            seed = int(seed)
            if seed < 0 or seed > 0xFFFFFFFF:
                raise ValueError('Seed must be between 0 and 2**32 - 1')
        self.ctx = ctx
        self.n = int(n)
        self.count = int(num_permutations)
        h = C.c_void_p()
        self.device_key = None
        if seed is None and device_stream_enabled() and int(movable.sum()) <= 65535:
            if shared and device_key is None:
                # a collective call: a key drawn here would differ from rank to rank and so would the tables
                raise ValueError('Permutations(seed=None, shared=True) needs a device_key the ranks agreed on '
                                 '(sharding.agree_on_seed / reduce_flags_and_stats)')
            self.device_key = int.from_bytes(os.urandom(8), 'little') if device_key is None else int(device_key) & 0xFFFFFFFFFFFFFFFF
            check(lib.safe_perms_create_device(ctx.handle, self.n, _ptr(movable), self.count, C.c_uint64(self.device_key), C.byref(h)))
        else:
            create = lib.safe_perms_create_shared if (shared and ctx.shared_stream) else lib.safe_perms_create
            check(create(ctx.handle, self.n, _ptr(movable), self.count, 0 if seed is None else 1,
                         0 if seed is None else seed, C.byref(h)))
        self.handle = h

    def timing(self):
        """Host-side timing of the stream (safe_perms_timing), ms, and this rank's role in it.  'resident': a seeded call that
        found the complete table of the previous identical call (same seed, n, count and movable rows) still on the device and
        drew nothing (SAFE_HIP_PERM_REUSE=0 switches that off)."""
        out = (C.c_double * 5)()
        check(lib.safe_perms_timing(self.handle, out))
        tw, ch, won = C.c_int(), C.c_int64(), C.c_int64()
        check(lib.safe_perms_twin_stats(self.handle, C.byref(tw), C.byref(ch), C.byref(won)))
        return {'draw_busy_ms': out[0], 'drawn_all_ms': out[1], 'tables_enqueued_ms': out[2], 'waited_for_producer_ms': out[3],
                'role': ('own', 'producer', 'consumer', 'device', 'resident')[int(out[4])],
                'twin_chain': bool(tw.value), 'chunks': ch.value, 'chunks_won_by_twin': won.value}

    @classmethod
    def from_table(cls, ctx, perm_idx):
        """Tables supplied by the caller instead of the legacy stream (safe_perms_create_from_table): perm_idx is
        [P, n], row p the COMPOSED index vector -- permuted matrix p = B[perm_idx[p]] (safe_extras.py:58 applied
        cumulatively).  Every row must be a permutation of 0..n-1."""
        perm_idx = np.ascontiguousarray(perm_idx, dtype=np.int32)
        if perm_idx.ndim != 2:
            raise ValueError('perm_idx must be [num_permutations, n]')
        self = cls.__new__(cls)
        self.ctx = ctx
        self.count, self.n = int(perm_idx.shape[0]), int(perm_idx.shape[1])
        h = C.c_void_p()
        check(lib.safe_perms_create_from_table(ctx.handle, self.n, self.count, _ptr(perm_idx), C.byref(h)))
        self.handle = h
        return self

    @classmethod
    def stratified(cls, ctx, n, movable, strata, num_permutations, key):
        """Restricted permutations generated on the device (safe_perms_create_device_strata): the movable rows are shuffled only
        inside their strata.  strata: int32 [n] labels >= 0, read where `movable` is set; key: 64 bits, None = OS entropy.  The
        tables are a function of (key, movable rows, partition, permutation index); one stratum gives the tables of
        Permutations(seed=None, device_key=key).  More than 65535 movable rows are refused."""
        movable = np.ascontiguousarray(movable, dtype=np.uint8)
        strata = np.ascontiguousarray(strata, dtype=np.int32)
        if movable.shape != (n,) or strata.shape != (n,):
            raise ValueError('movable and strata must have one entry per row (%d)' % n)
        self = cls.__new__(cls)
        self.ctx = ctx
        self.n, self.count = int(n), int(num_permutations)
        self.handle = None
        self.device_key = int.from_bytes(os.urandom(8), 'little') if key is None else int(key) & 0xFFFFFFFFFFFFFFFF
        h = C.c_void_p()
        check(lib.safe_perms_create_device_strata(ctx.handle, self.n, _ptr(movable), _ptr(strata), self.count,
                                                  C.c_uint64(self.device_key), C.byref(h)))
        self.handle = h
        return self

    def slice(self, p0, p1):
        """Permutations [p0, p1) as a handle of their own (safe_perms_slice): one rank's range of a permutation-axis split."""
        other = Permutations.__new__(Permutations)
        other.ctx, other.n, other.count = self.ctx, self.n, int(p1) - int(p0)
        h = C.c_void_p()
        check(lib.safe_perms_slice(self.handle, int(p0), int(p1), C.byref(h)))
        other.handle = h
        return other

    def read(self, p0=0, p1=None):
        p1 = self.count if p1 is None else p1
        out = np.empty((p1 - p0, self.n), dtype=np.int32)
        check(lib.safe_perms_read(self.handle, p0, p1, _ptr(out)))
        return out

    def close(self):
        if self.handle:
            check(lib.safe_perms_destroy(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """RCCL communicator behind the C ABI (safe_comm_* / safe_allgather_cols): the final exchange of the
    attribute-sharded path for hosts without torch.distributed.  `Comm.unique_id()` on one rank, the 128 bytes to
    every rank by any means, then `Comm(ctx, world, rank, uid)` on each (one GPU per rank)."""

    ID_BYTES = 128

    @staticmethod
    def _framework_first():
        """When PyTorch-ROCm is installed its bundled RCCL must be the process's RCCL, loaded the way torch loads it:
        dlopen-ing that file ahead of `import torch` (or a second copy beside it) ends in a heap corruption at interpreter
        exit.  A host without torch uses the system's librccl (comm.cpp)."""
        try:
            import torch  # noqa: F401
        except ImportError:
            pass

    @staticmethod
    def unique_id():
        Comm._framework_first()
        buf = C.create_string_buffer(Comm.ID_BYTES)
        check(lib.safe_comm_unique_id(buf, Comm.ID_BYTES))
        return buf.raw

    def __init__(self, ctx, world_size, rank, unique_id):
        assert len(unique_id) == self.ID_BYTES
        self._framework_first()
        self.ctx, self.world_size, self.rank = ctx, int(world_size), int(rank)
        h = C.c_void_p()
        check(lib.safe_comm_create(ctx.handle, self.world_size, self.rank, unique_id, self.ID_BYTES, C.byref(h)))
        self.handle = h

    def allgather(self, local_ptr, bytes_per_rank, all_ptr):
        """Enqueue (context stream) the all-gather of every rank's `bytes_per_rank` bytes at device pointer
        `local_ptr` into `all_ptr` (world_size slabs in rank order)."""
        check(lib.safe_allgather_cols(self.handle, C.c_void_p(local_ptr), int(bytes_per_rank), C.c_void_p(all_ptr)))

    def close(self):
        if self.handle:
            check(lib.safe_comm_destroy(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_stream_enabled():
    """Unseeded runs generate their permutation tables on the device unless SAFE_HIP_DEVICE_STREAM=0."""
    return os.environ.get('SAFE_HIP_DEVICE_STREAM', '1') != '0'


def effective_cores():
    """CPUs this process may actually use: the scheduler affinity, capped by the container's CFS quota (cgroup v2 cpu.max /
    v1 cfs_quota_us) when there is one."""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if quota != 'max':
            cores = min(cores, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            quota = int(open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us').read())
            period = int(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
            if quota > 0:
                cores = min(cores, max(1, quota // period))
        except (OSError, ValueError):
            pass
    return cores


def configure_host_for_ranks(local_world):
    """Host-side settings of one rank among `local_world` on this node, BEFORE its Context exists: when a rank has fewer than
    three cores to itself its host waits sleep instead of spinning (a spinning launcher + draw thread per rank on a 16-CPU
    quota gets the whole job throttled).  The only host thread of the permutation stream is the draw thread of a seeded
    call (one per node when the stream is shared); the swaps are replayed on the device.
    Environment override: SAFE_HIP_BLOCKING_SYNC.  Returns what was chosen."""
    local_world = max(1, int(local_world))
    share = effective_cores() / local_world
    blocking = os.environ.get('SAFE_HIP_BLOCKING_SYNC')
    blocking = (share < 3) if blocking is None else (blocking not in ('0', ''))
    set_blocking_sync(blocking)
    return {'cores_per_rank': share, 'blocking_sync': bool(blocking)}


def set_blocking_sync(on):
    """Host waits sleep on interrupt-backed events instead of spinning (safe_set_blocking_sync); before the first Context."""
    check(lib.safe_set_blocking_sync(1 if on else 0))


def device_alloc_count():
    """hipMalloc / hipHostMalloc calls the library has made in this process so far (safe_alloc_count)."""
    v = C.c_int64()
    check(lib.safe_alloc_count(C.byref(v)))
    return v.value


def device_live_alloc_count():
    """Device blocks the library holds in this process right now (safe_live_alloc_count): the same before and after a call
    that returns no handle, once the context's scratch has grown to the call's shape."""
    v = C.c_int64()
    check(lib.safe_live_alloc_count(C.byref(v)))
    return v.value


def last_mfma_slices(ctx):
    """i8 slices the last matrix-core permutation test ran with (2 / 4 / 6; 0 = it has not run)."""
    v = C.c_int()
    check(lib.safe_last_mfma_slices(ctx.handle, C.byref(v)))
    return v.value


def build_info():
    """Compiler version and build-time checks of the loaded library."""
    buf = C.create_string_buffer(512)
    check(lib.safe_build_info(buf, 512))
    return buf.value.decode()


def last_mfma_filter(ctx):
    """(slices the matrix cores multiplied, compares settled from the low digits) of the last matrix-core permutation test;
    a negative second value: the undecided list overflowed and the call was repeated with all six slices."""
    s, u = C.c_int(), C.c_int64()
    check(lib.safe_last_mfma_filter(ctx.handle, C.byref(s), C.byref(u)))
    return s.value, u.value


def rng_permutations_host(seed, values, count):
    """Host-only: `count` successive np.random.permutation(values) draws after np.random.seed(seed)."""
    values = np.ascontiguousarray(values, dtype=np.int64)
    out = np.empty((count, values.shape[0]), dtype=np.int64)
    check(lib.safe_rng_permutations_host(int(seed), _ptr(values), values.shape[0], int(count), _ptr(out)))
    return out


def nes_table(num_permutations):
    """-log10 of every possible empirical p-value k/P (k=0 -> 1/P), evaluated with NumPy so
    NES equals the reference's np.log10 bit for bit (safepy/safe.py:546-547)."""
    p = np.arange(num_permutations + 1, dtype=np.float64) / num_permutations
    with np.errstate(divide='ignore'):
        return np.ascontiguousarray(-np.log10(np.where(p == 0, 1 / num_permutations, p)))


# ---- enrichment entry points on device buffers -----------------------------------------

def score(ctx, nbr, attr, score_type, out_ptr, col0=0, col1=None):
    col1 = attr.m if col1 is None else col1
    check(lib.safe_score(ctx.handle, nbr.handle, attr.handle, _SCORE[score_type], col0, col1, C.c_void_p(out_ptr)))


def permtest_counts(ctx, nbr, attr, perms, score_type, ns_ptr, neg_ptr, pos_ptr, col0=0, col1=None):
    col1 = attr.m if col1 is None else col1
    check(lib.safe_permtest_counts(ctx.handle, nbr.handle, attr.handle, perms.handle, _SCORE[score_type], col0, col1,
                                   C.c_void_p(ns_ptr) if ns_ptr else None, C.c_void_p(neg_ptr), C.c_void_p(pos_ptr)))


def randomization(ctx, nbr, attr, perms, score_type, attribute_sign, enrichment_threshold, out_ptrs,
                  col0=0, col1=None, table=None):
    """out_ptrs = (ns, pvalues_neg, pvalues_pos, nes, nes_binary, num_enriched) device pointers."""
    col1 = attr.m if col1 is None else col1
    if table is None:
        table = nes_table(perms.count)
    ns, pn, pp, nes, nb, ne = out_ptrs
    check(lib.safe_randomization(ctx.handle, nbr.handle, attr.handle, perms.handle, _SCORE[score_type],
                                 _SIGN[attribute_sign], float(enrichment_threshold), _ptr(table), col0, col1,
                                 C.c_void_p(ns) if ns else None, C.c_void_p(pn), C.c_void_p(pp), C.c_void_p(nes),
                                 C.c_void_p(nb), C.c_void_p(ne)))


def outputs_from_counts(ctx, n, m, num_permutations, attribute_sign, enrichment_threshold, counts_neg_ptr, counts_pos_ptr, ns_ptr,
                        out_ptrs, table=None):
    """#<= / #>= counts of a whole call (f64 [n, m] on the device) -> out_ptrs = (pvalues_neg, pvalues_pos, nes, nes_binary,
    num_enriched) device pointers (safe_outputs_from_counts; safe.py:528-554, 468-472)."""
    if table is None:
        table = nes_table(num_permutations)
    pn, pp, nes, nb, ne = out_ptrs
    check(lib.safe_outputs_from_counts(ctx.handle, int(n), int(m), int(num_permutations), _SIGN[attribute_sign],
                                       float(enrichment_threshold), _ptr(table), C.c_void_p(counts_neg_ptr), C.c_void_p(counts_pos_ptr),
                                       C.c_void_p(ns_ptr) if ns_ptr else None, C.c_void_p(pn), C.c_void_p(pp), C.c_void_p(nes),
                                       C.c_void_p(nb), C.c_void_p(ne)))


def hypergeom(ctx, nbr, attr, enrichment_threshold, out_ptrs, col0=0, col1=None):
    """out_ptrs = (pvalues_pos, nes, nes_binary, num_enriched) device pointers."""
    col1 = attr.m if col1 is None else col1
    pp, nes, nb, ne = out_ptrs
    check(lib.safe_hypergeom(ctx.handle, nbr.handle, attr.handle, float(enrichment_threshold), col0, col1,
                             C.c_void_p(pp), C.c_void_p(nes), C.c_void_p(nb), C.c_void_p(ne)))


HYP_EVALUATORS = {None: 0, 'auto': 0, 'table': 1, 'element': 2}


def hypergeom_tails(ctx, nbr, attr, attribute_sign, enrichment_threshold, out_ptrs, col0=0, col1=None, evaluator=None):
    """Both hypergeometric tails of 0/1 attributes: out_ptrs = (ns, pvalues_neg, pvalues_pos, nes, nes_binary, num_enriched)
    device pointers.  evaluator: None / 'auto' (the library chooses), 'table', 'element'."""
    col1 = attr.m if col1 is None else col1
    check(lib.safe_hypergeom_tails(ctx.handle, nbr.handle, attr.handle, _SIGN[attribute_sign], float(enrichment_threshold),
                                   HYP_EVALUATORS[evaluator], col0, col1, *[C.c_void_p(p) if p else None for p in out_ptrs]))


def hypergeom_outputs(ctx, n, m, attribute_sign, enrichment_threshold, pvalues_neg_ptr, pvalues_pos_ptr, out_ptrs):
    """NES, nes_binary and the enriched counts from two p matrices: out_ptrs = (nes, nes_binary, num_enriched)."""
    check(lib.safe_hypergeom_outputs(ctx.handle, int(n), int(m), _SIGN[attribute_sign], float(enrichment_threshold),
                                     *[C.c_void_p(p) if p else None for p in (pvalues_neg_ptr, pvalues_pos_ptr) + tuple(out_ptrs)]))


def moments_test(ctx, nbr, attr, attribute_sign, enrichment_threshold, out_ptrs, col0=0, col1=None, z_ptr=None):
    """The analytic test of 'sum' scores (exact permutation moments, normal tails; safe_moments_test): out_ptrs = (ns,
    pvalues_neg, pvalues_pos, nes, nes_binary, num_enriched) device pointers; z_ptr: where the z matrix goes, or None."""
    col1 = attr.m if col1 is None else col1
    check(lib.safe_moments_test(ctx.handle, nbr.handle, attr.handle, _SIGN[attribute_sign], float(enrichment_threshold), col0, col1,
                                *[C.c_void_p(p) if p else None for p in tuple(out_ptrs) + (z_ptr,)]))


def score_weighted(ctx, nbr, attr, out_ptr, col0=0, col1=None):
    """The weighted 'sum' score of a handle that carries weights (safe_score_weighted): f64 [n, col1 - col0] at out_ptr."""
    col1 = attr.m if col1 is None else col1
    check(lib.safe_score_weighted(ctx.handle, nbr.handle, attr.handle, col0, col1, C.c_void_p(out_ptr)))


def moments_test_weighted(ctx, nbr, attr, attribute_sign, enrichment_threshold, out_ptrs, col0=0, col1=None, z_ptr=None):
    """moments_test for the weighted score (safe_moments_test_weighted): the same out_ptrs and z_ptr."""
    col1 = attr.m if col1 is None else col1
    check(lib.safe_moments_test_weighted(ctx.handle, nbr.handle, attr.handle, _SIGN[attribute_sign], float(enrichment_threshold), col0,
                                         col1, *[C.c_void_p(p) if p else None for p in tuple(out_ptrs) + (z_ptr,)]))


def permtest_counts_weighted(ctx, nbr, attr, perms, ns_ptr, neg_ptr, pos_ptr, col0=0, col1=None):
    """permtest_counts for the weighted 'sum' score (safe_permtest_counts_weighted); ns_ptr may be None."""
    col1 = attr.m if col1 is None else col1
    check(lib.safe_permtest_counts_weighted(ctx.handle, nbr.handle, attr.handle, perms.handle, col0, col1,
                                            C.c_void_p(ns_ptr) if ns_ptr else None, C.c_void_p(neg_ptr), C.c_void_p(pos_ptr)))


# familywise_scope -> SAFE_FAMILY_*: the family whose extreme every observed statistic is compared with
FAMILY_SCOPES = {'neighborhoods': _lib.FAMILY_COLUMN, 'all': _lib.FAMILY_MATRIX}


def permtest_extremes(ctx, nbr, attr, perms, z_ptr, live_ptr, tmax_ptr, tmin_ptr, col0=0, col1=None):
    """Per permutation and column, the extremes over the rows of the standardised permuted 'sum' scores
    (safe_permtest_extremes): tmax / tmin f64 [P, col1 - col0]; z_ptr (f64) and live_ptr (u8), each [n, col1 - col0] or None:
    the observed statistic and the flags of the non-degenerate cells.  Flat and weighted handles."""
    col1 = attr.m if col1 is None else col1
    check(lib.safe_permtest_extremes(ctx.handle, nbr.handle, attr.handle, perms.handle, col0, col1,
                                     *[C.c_void_p(p) if p else None for p in (z_ptr, live_ptr, tmax_ptr, tmin_ptr)]))


def counts_from_extremes(ctx, n, m, num_permutations, scope, z_ptr, live_ptr, tmax_ptr, tmin_ptr, neg_ptr, pos_ptr,
                         min_neg_ptr=None, min_pos_ptr=None):
    """The max-statistic adjusted counts (safe_counts_from_extremes): scope 'neighborhoods' or 'all' (or a SAFE_FAMILY_* value);
    counts f64 [n, m] at neg_ptr / pos_ptr, the columns' smallest counts f64 [m] at min_neg_ptr / min_pos_ptr (or None)."""
    check(lib.safe_counts_from_extremes(ctx.handle, int(n), int(m), int(num_permutations), int(FAMILY_SCOPES.get(scope, scope)),
                                        *[C.c_void_p(p) if p else None for p in (z_ptr, live_ptr, tmax_ptr, tmin_ptr, neg_ptr, pos_ptr,
                                                                                 min_neg_ptr, min_pos_ptr)]))


def fdr_adjust_rows(ctx, n, m, p_ptr):
    """Benjamini-Hochberg on every row of one f64 [n, m] device matrix, in place."""
    check(lib.safe_fdr_adjust_rows(ctx.handle, int(n), int(m), C.c_void_p(p_ptr) if p_ptr else None))


# multiple_testing_scope -> SAFE_FDR_SCOPE_*: the family one Benjamini-Hochberg run adjusts
FDR_SCOPES = {'attributes': _lib.FDR_SCOPE_ROWS, 'neighborhoods': _lib.FDR_SCOPE_COLS, 'all': _lib.FDR_SCOPE_ALL}


def _fdr_scope(scope):
    return FDR_SCOPES[scope] if isinstance(scope, str) else int(scope)


def fdr_adjust_matrix(ctx, n, m, scope, p_ptr, count_denominator=0):
    """Benjamini-Hochberg on one f64 [n, m] device matrix, in place, along `scope` ('attributes': rows, 'neighborhoods': columns,
    'all': the whole matrix; or a SAFE_FDR_SCOPE_* number).  count_denominator = P > 0: the entries are counts / P (checked; the
    histogram forms); 0: the families are sorted."""
    check(lib.safe_fdr_adjust_matrix(ctx.handle, int(n), int(m), _fdr_scope(scope), int(count_denominator),
                                     C.c_void_p(p_ptr) if p_ptr else None))


def fdr_adjust_scope(ctx, n, m, num_permutations, attribute_sign, enrichment_threshold, scope, out_ptrs):
    """fdr_adjust with the family named by `scope` (see fdr_adjust_matrix): out_ptrs = (pvalues_neg or None, pvalues_pos, nes,
    nes_binary, num_enriched); num_permutations = 0 selects the hypergeometric form."""
    check(lib.safe_fdr_adjust_scope(ctx.handle, int(n), int(m), int(num_permutations), _SIGN[attribute_sign], float(enrichment_threshold),
                                    _fdr_scope(scope), *[C.c_void_p(p) if p else None for p in out_ptrs]))


# multiple_testing_method -> SAFE_MT_*: the procedure that adjusts a family (statsmodels' multipletests names)
MT_METHODS = {'fdr_bh': _lib.MT_FDR_BH, 'fdr_by': _lib.MT_FDR_BY, 'holm': _lib.MT_HOLM, 'hochberg': _lib.MT_HOCHBERG,
              'bonferroni': _lib.MT_BONFERRONI}
_BY_CHUNK = 1 << 24
_by_constants = {}


def by_constant(count):
    """Benjamini-Yekutieli's constant of a family of `count` tests, sum_{i <= count} 1 / i, as a float: statsmodels' own
    expression np.sum(1. / np.arange(1, count + 1)) up to 2^24 terms; beyond that the same expression on chunks of at most 2^24
    terms, the chunk sums joined with math.fsum (a 2 10^8-cell matrix does not allocate gigabytes).  Cached per count."""
    count = int(count)
    if count < 1:
        raise ValueError('by_constant: a family has at least one test, not %d' % count)
    if count not in _by_constants:
        if count <= _BY_CHUNK:
            value = float(np.sum(1. / np.arange(1, count + 1)))
        else:
            value = math.fsum(float(np.sum(1. / np.arange(lo, min(lo + _BY_CHUNK, count + 1))))
                              for lo in range(1, count + 1, _BY_CHUNK))
        _by_constants[count] = value
    return _by_constants[count]


def _mt_method(method, n, m, scope):
    """(SAFE_MT_* number, by_constant of the scope's family or 0.0)"""
    method = MT_METHODS[method] if isinstance(method, str) else int(method)
    if method != _lib.MT_FDR_BY:
        return method, 0.0
    scope = _fdr_scope(scope)
    count = {_lib.FDR_SCOPE_ROWS: int(m), _lib.FDR_SCOPE_COLS: int(n), _lib.FDR_SCOPE_ALL: int(n) * int(m)}.get(scope, 0)
    return method, by_constant(count) if count >= 1 else 1.0        # (sizes and scopes the library refuses: it names them)


def mt_adjust_matrix(ctx, n, m, scope, method, p_ptr, count_denominator=0, by_const=None):
    """fdr_adjust_matrix with the procedure `method` ('fdr_bh', 'fdr_by', 'holm', 'hochberg', 'bonferroni', or a SAFE_MT_* number);
    by_const: Benjamini-Yekutieli's constant, by default by_constant of the scope's family."""
    number, c = _mt_method(method, n, m, scope) if by_const is None else (MT_METHODS.get(method, method), by_const)
    check(lib.safe_mt_adjust_matrix(ctx.handle, int(n), int(m), _fdr_scope(scope), int(number), float(c), int(count_denominator),
                                    C.c_void_p(p_ptr) if p_ptr else None))


def mt_adjust_scope(ctx, n, m, num_permutations, attribute_sign, enrichment_threshold, scope, method, out_ptrs, by_const=None):
    """fdr_adjust_scope with the procedure `method` (see mt_adjust_matrix)."""
    number, c = _mt_method(method, n, m, scope) if by_const is None else (MT_METHODS.get(method, method), by_const)
    check(lib.safe_mt_adjust_scope(ctx.handle, int(n), int(m), int(num_permutations), _SIGN[attribute_sign], float(enrichment_threshold),
                                   _fdr_scope(scope), int(number), float(c), *[C.c_void_p(p) if p else None for p in out_ptrs]))


def packed_counts_info(ctx):
    """(n_pad, m, layout) of the integer counters the last randomization call left on the device;
    layout -1 = none (f64 kernels)."""
    n_pad, m, layout = C.c_int64(), C.c_int64(), C.c_int()
    check(lib.safe_export_packed_counts(ctx.handle, None, 0, C.byref(n_pad), C.byref(m), C.byref(layout)))
    return n_pad.value, m.value, layout.value


def export_packed_counts(ctx, dst_ptr, capacity):
    n_pad, m, layout = C.c_int64(), C.c_int64(), C.c_int()
    check(lib.safe_export_packed_counts(ctx.handle, C.c_void_p(dst_ptr), int(capacity), C.byref(n_pad), C.byref(m),
                                        C.byref(layout)))
    return n_pad.value, m.value, layout.value


_ENQUEUED_FN = C.CFUNCTYPE(None, C.c_void_p)


def set_exchange_chunks(ctx, chunks, cols_per_chunk=0, on_enqueued=None):
    """Arms (chunks >= 2) or switches off (0) the column-chunked tail of the following randomization calls on `ctx`
    (safe_set_exchange_chunks).  `on_enqueued()` is called on the calling thread, inside the randomization call, once all
    of its launches are enqueued.  An exception it raises is kept and re-raised by take_exchange_error()."""
    if not chunks:
        check(lib.safe_set_exchange_chunks(ctx.handle, 0, 0, None, None))
        ctx._xc_cb = None
        return
    ctx._xc_error = None

    def trampoline(_user):
        try:
            if on_enqueued is not None:
                on_enqueued()
        except BaseException as err:           # (an exception cannot cross the C frames of the call)
            ctx._xc_error = err
    cb = _ENQUEUED_FN(trampoline)
    ctx._xc_cb = cb                             # the library keeps the raw pointer: the object must outlive the calls
    check(lib.safe_set_exchange_chunks(ctx.handle, int(chunks), int(cols_per_chunk), C.cast(cb, C.c_void_p), None))


def take_exchange_error(ctx):
    err, ctx._xc_error = getattr(ctx, '_xc_error', None), None
    if err is not None:
        raise err


def packed_chunk_info(ctx):
    """(chunks, [column bounds], tail permutations) of the last randomization call; chunks = 0: it ran no column-chunked launches."""
    k, tail = C.c_int(), C.c_int64()
    bounds = (C.c_int64 * 9)()
    check(lib.safe_packed_chunk_info(ctx.handle, C.byref(k), bounds, C.byref(tail)))
    return k.value, [bounds[i] for i in range(k.value + 1)] if k.value else [], tail.value


PACKED_NARROW = 16          # safe_hip.h SAFE_PACKED_NARROW: slabs of 20-bit counter pairs (num_permutations <= 1023)


def packed_slab_words(cols, n_pad, narrow):
    """u32 words of a slab of `cols` columns of packed counters: n_pad per column, or 5 n_pad / 8 in the narrow form."""
    return int(cols) * (int(n_pad) // 8 * 5 if narrow else int(n_pad))


def export_packed_chunk(ctx, chunk, dst_ptr, capacity, stream=None, narrow=False):
    """Chunk `chunk` of the last randomization call's counters to dst_ptr (`capacity` u32 words, the rest zeroed) on `stream`;
    narrow: two outputs in five bytes (safe_export_packed_chunk_narrow, num_permutations <= 1023)."""
    fn = lib.safe_export_packed_chunk_narrow if narrow else lib.safe_export_packed_chunk
    check(fn(ctx.handle, int(chunk), C.c_void_p(dst_ptr), int(capacity), C.c_void_p(stream) if stream else None))


def outputs_from_packed_slabs(ctx, nbr, slabs_ptr, layout, n_pad, slab_stride, slab_cols, out_col0, m_total, num_permutations,
                              attribute_sign, enrichment_threshold, out_ptrs, table=None, stream=None):
    """out_ptrs = (pvalues_neg, pvalues_pos, nes, nes_binary) device pointers of f64 [n, m_total] matrices (None = not wanted);
    slab r = slab_cols[r] columns of u32 counters at slabs_ptr + 4 * r * slab_stride, written to columns out_col0[r] ...
    (safe_outputs_from_packed_slabs); enqueued on `stream` (a raw hipStream_t; None: the context's), not waited for."""
    if table is None:
        table = nes_table(num_permutations)
    k = len(slab_cols)
    cols = (C.c_int64 * k)(*[int(v) for v in slab_cols])
    col0 = (C.c_int64 * k)(*[int(v) for v in out_col0])
    pn, pp, nes, nb = (C.c_void_p(p) if p else None for p in out_ptrs)
    check(lib.safe_outputs_from_packed_slabs(ctx.handle, nbr.handle, C.c_void_p(slabs_ptr), int(layout), int(n_pad), k, int(slab_stride),
                                             cols, col0, int(m_total), int(num_permutations), _SIGN[attribute_sign],
                                             float(enrichment_threshold), _ptr(table), pn, pp, nes, nb,
                                             C.c_void_p(stream) if stream else None))


def randomization_plan(ctx, nbr, attr, num_permutations, score_type):
    """The packed-counter layout safe_randomization would leave for this block (0 = bit-sliced kernel), -1 = none predicted."""
    layout = C.c_int()
    check(lib.safe_randomization_plan(ctx.handle, nbr.handle, attr.handle, int(num_permutations), _SCORE[score_type], C.byref(layout)))
    return layout.value


def nes_from_packed_counts(ctx, nbr, counts_ptr, layout, n_pad, m, num_permutations, attribute_sign, nes_ptr, table=None):
    if table is None:
        table = nes_table(num_permutations)
    check(lib.safe_nes_from_packed_counts(ctx.handle, nbr.handle, C.c_void_p(counts_ptr), int(layout), int(n_pad), int(m),
                                          int(num_permutations), _SIGN[attribute_sign], _ptr(table), C.c_void_p(nes_ptr)))


def outputs_from_packed_counts(ctx, nbr, counts_ptr, layout, n_pad, m, num_permutations, attribute_sign, enrichment_threshold,
                               out_ptrs, table=None):
    """out_ptrs = (pvalues_neg, pvalues_pos, nes, nes_binary) device pointers of f64 [n, m] matrices, None = not wanted
    (safe_outputs_from_packed_counts)."""
    if table is None:
        table = nes_table(num_permutations)
    pn, pp, nes, nb = (C.c_void_p(p) if p else None for p in out_ptrs)
    check(lib.safe_outputs_from_packed_counts(ctx.handle, nbr.handle, C.c_void_p(counts_ptr), int(layout), int(n_pad), int(m),
                                              int(num_permutations), _SIGN[attribute_sign], float(enrichment_threshold), _ptr(table),
                                              pn, pp, nes, nb))


def block_count(nbr):
    """Stored 256 x 32 blocks of the block-sparse membership the matrix-core kernel multiplies
    (built on first use by that kernel; 0 before)."""
    c = C.c_int64()
    check(lib.safe_nbr_block_count(nbr.handle, C.byref(c)))
    return c.value


def piece_count(nbr):
    """32 x 32 pieces of the stored membership blocks that hold a member: the ones the matrix-core kernel multiplies (safe_nbr_piece_count)."""
    v = C.c_int64()
    check(lib.safe_nbr_piece_count(nbr.handle, C.byref(v)))
    return v.value


def fdr_adjust(ctx, n, m, num_permutations, attribute_sign, enrichment_threshold, out_ptrs):
    """multiple_testing=True: out_ptrs = (pvalues_neg or None, pvalues_pos, nes, nes_binary, num_enriched);
    num_permutations = 0 selects the hypergeometric form."""
    pn, pp, nes, nb, ne = out_ptrs
    check(lib.safe_fdr_adjust(ctx.handle, int(n), int(m), int(num_permutations), _SIGN[attribute_sign],
                              float(enrichment_threshold), C.c_void_p(pn) if pn else None, C.c_void_p(pp), C.c_void_p(nes),
                              C.c_void_p(nb), C.c_void_p(ne)))


def enriched_components(ctx, n, edge_u, edge_v, member):
    """member: [n, n_cols] (> 0 = enriched).  Returns int32 [n_cols, n] component labels (smallest
    node id of the component; -1 = not enriched) -- safe.py:640-655 for all attributes at once."""
    member = np.ascontiguousarray(member, dtype=np.float64)
    assert member.ndim == 2 and member.shape[0] == n
    eu, ev, _ = _edges(edge_u, edge_v, None, 'enriched_components')
    out = np.empty((member.shape[1], n), dtype=np.int32)
    check(lib.safe_enriched_components(ctx.handle, int(n), eu.shape[0], _ptr(eu), _ptr(ev), _ptr(member), member.shape[1], _ptr(out)))
    return out


def enriched_pair_counts(ctx, nbr, member):
    """member: [n, n_cols] (> 0 = enriched), n = nbr.n.  Returns (q, e), int64 [n_cols] each: e[a] = the enriched nodes of column
    a, q[a] = the sum of nbr's membership W[i, j] over the ordered pairs (i, j) of them, the diagonal included
    (safe_enriched_pair_counts).  For a symmetric W with a full diagonal (q - e) // 2 pairs i < j are within reach."""
    member = np.ascontiguousarray(member, dtype=np.float64)
    if member.ndim != 2 or member.shape[0] != nbr.n:
        raise ValueError('enriched_pair_counts: member of shape %s for %d nodes' % (member.shape, nbr.n))
    q = np.empty(member.shape[1], dtype=np.int64)
    e = np.empty(member.shape[1], dtype=np.int64)
    check(lib.safe_enriched_pair_counts(ctx.handle, nbr.handle, _ptr(member), member.shape[1], _ptr(q), _ptr(e)))
    return q, e


def jaccard_condensed(ctx, x):
    """scipy pdist(x, 'jaccard') (condensed) for the rows of x [m_top, n]."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    m_top, n = x.shape
    out = np.empty(m_top * (m_top - 1) // 2, dtype=np.float64)
    check(lib.safe_jaccard_condensed(ctx.handle, m_top, n, _ptr(x), _ptr(out)))
    return out


def pair_distance_select(ctx, xy, ranks):
    """Context.pair_distance_select: (values [len(ranks)], number of pairs)."""
    return ctx.pair_distance_select(xy, ranks)


def nbr_distance_select(nbr, ranks):
    """Neighborhoods.distance_select: (values [len(ranks)], number of finite pairs)."""
    return nbr.distance_select(ranks)


def kde_grid(ctx, offsets, pts, weights, norm, xi):
    """Context.kde_grid: (z [D, G], kernel ms)."""
    return ctx.kde_grid(offsets, pts, weights, norm, xi)


def domain_counts(ctx, values, domain, n_domains, n=None, m=None):
    """Context.domain_counts: (counts [n, n_domains], kernel ms)."""
    return ctx.domain_counts(values, domain, n_domains, n, m)


def gather_columns(ctx, values, cols, n=None, m=None):
    """Context.gather_columns: (columns [n, k], kernel ms)."""
    return ctx.gather_columns(values, cols, n, m)


def enriched_components_dev(ctx, values_dev_ptr, n, m, cols, edge_u, edge_v):
    """Context.enriched_components_dev: (labels int32 [len(cols), n], kernel ms)."""
    return ctx.enriched_components_dev(values_dev_ptr, n, m, cols, edge_u, edge_v)


def enriched_pair_counts_dev(ctx, nbr, values_dev_ptr, n, m, cols):
    """Context.enriched_pair_counts_dev: (q, e, kernel ms)."""
    return ctx.enriched_pair_counts_dev(nbr, values_dev_ptr, n, m, cols)


def profile_distances(ctx, values_dev_ptr, n, m, cols, metric):
    """Context.profile_distances: (condensed distances, kernel ms)."""
    return ctx.profile_distances(values_dev_ptr, n, m, cols, metric)


def linkage_average(ctx, cond, m_top=None):
    """Context.linkage_average: (Z [m_top - 1, 4], kernel ms)."""
    return ctx.linkage_average(cond, m_top)


def profile_linkage(ctx, values_dev_ptr, n, m, cols, metric):
    """Context.profile_linkage: (Z [len(cols) - 1, 4], kernel ms)."""
    return ctx.profile_linkage(values_dev_ptr, n, m, cols, metric)


def node_domains(ctx, nes_binary_dev_ptr, nes_dev_ptr, n, m, domain, ids):
    """Context.node_domains: (sums [n, len(ids)], primary int32 [n], primary_nes [n], kernel ms)."""
    return ctx.node_domains(nes_binary_dev_ptr, nes_dev_ptr, n, m, domain, ids)


def enriched_pairs(ctx, selector_ptr, values_ptr, n, m, mode, threshold, axis):
    """Context.enriched_pairs: (indptr int32, indices int32 [nnz], data f64 [nnz] or None, (count ms, emit ms))."""
    return ctx.enriched_pairs(selector_ptr, values_ptr, n, m, mode, threshold, axis)
