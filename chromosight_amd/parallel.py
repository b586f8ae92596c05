"""Multi-GPU driver of the hot path: one process per GPU, sub-matrices sharded across ranks,
candidate records gathered at the end.

Mirrors the only parallelism of the reference -- `multiprocessing.Pool(threads).imap` over
independent sub-matrices, one task = one sub-matrix x one kernel
(reference chromosight/cli/chromosight.py:406-410, 748-752) -- with `torch.distributed`
(backend "nccl" = RCCL over xGMI on the GPU box, "gloo" in CPU tests).  Sub-matrices are
independent (own distance law, mask and foci), so the data path has no collective; the only
exchange is the final gather of the per-block pattern tables (a few MB at most).

    tables = detect_blocks(blocks, kernel_config, kernel_matrix, detector=...)

`blocks` is a list of objects with the attributes pattern_detector reads (`matrix`,
`detectable_bins`, `max_dist`, `inter`); every rank passes the same list (or builds the same
list lazily through `loader`), processes its own share and receives the gathered result.
"""
import os
import sys

import numpy as np

RECORD_FIELDS = ("block", "bin1", "bin2", "score", "pvalue")


def block_cost(shape, max_dist, inter):
    """Pixels the correlation scans for one sub-matrix (SURVEY.md 8(d) unit of work)."""
    rows, cols = shape
    if inter or max_dist is None:
        return int(rows) * int(cols)
    return int(rows) * int(min(max_dist + 1, cols))


def assign_blocks(costs, world_size):
    """Longest-processing-time-first assignment of blocks to ranks.  Returns a list with, for
    every rank, the (sorted) indices of its blocks; deterministic, identical on every rank."""
    order = sorted(range(len(costs)), key=lambda i: (-costs[i], i))
    load = [0] * world_size
    owned = [[] for _ in range(world_size)]
    for i in order:
        r = min(range(world_size), key=lambda k: (load[k], k))
        owned[r].append(i)
        load[r] += costs[i]
    return [sorted(o) for o in owned]


_COMMS = {}


class NativeComm:
    """The library's RCCL communicator (csrc/cs_comm.cpp: ncclAllGather / ncclAllReduce behind the C ABI, host arrays in
    and out, no torch tensors in the exchange)."""

    def __init__(self, device, rank, world, unique_id):
        import ctypes as C
        from ._lib import load_library
        self.C, self.lib = C, load_library()
        self.rank, self.world = rank, world
        self.handle = C.c_void_p()
        rc = self.lib.cs_comm_create(int(device), int(rank), int(world), unique_id, C.byref(self.handle))
        if rc != 0:
            raise RuntimeError(f"cs_comm_create failed ({rc}): {self.lib.cs_comm_last_error(None).decode()}")

    @staticmethod
    def unique_id():
        import ctypes as C
        from ._lib import load_library
        buf = (C.c_char * 128)()
        rc = load_library().cs_comm_unique_id(buf)
        if rc != 0:
            raise RuntimeError(f"cs_comm_unique_id failed ({rc})")
        return bytes(buf)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"RCCL exchange failed ({rc}): {self.lib.cs_comm_last_error(self.handle).decode()}")

    def allgather_rows(self, rows, first_cap=0):
        """Rank-order concatenation of every rank's (n_i, w) float64 array, and the per-rank counts.  first_cap: this rank's
        first capacity in rows (0: a guess from its own count) -- the self-check hands a small one so that the retry runs."""
        C = self.C
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        width = int(rows.shape[1])
        counts = np.zeros(self.world, dtype=np.int64)
        # first guess; CHROMOSIGHT_HIP_GATHER_CAP forces a small one (tests of the retry).  The library exchanges the
        # capacities with the counts and answers "overflow" on EVERY rank when any rank lacks room, so all ranks retry
        # together with the exact total (the collectives stay matched whatever the per-rank guesses were).
        cap = int(first_cap) or int(os.environ.get("CHROMOSIGHT_HIP_GATHER_CAP", 0)) or max(4 * rows.shape[0] * self.world, 4096)
        while True:
            out = np.empty((cap, width))
            rc = self.lib.cs_comm_allgather_rows(self.handle, rows.ctypes.data, rows.shape[0], width, out.ctypes.data, cap,
                                                 counts.ctypes.data)
            if rc == -4:                      # CS_ERR_OVERFLOW: the counts say how much room is needed
                cap = int(counts.sum())
                continue
            self._check(rc)
            return out[:int(counts.sum())], counts

    def allgather_rows_once(self, rows):
        """allgather_rows in ONE collective (cs_comm_allgather_rows_once): the slot is what the previous exchange of this width
        needed, with a quarter to spare -- a step of a sharded run finds about as many records as the step before; a list that
        outgrows it makes every rank call again with the longest list as the slot."""
        C = self.C
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        width = int(rows.shape[1])
        counts = np.zeros(self.world, dtype=np.int64)
        slots = self.__dict__.setdefault("_slots", {})
        slot = slots.get(width) or int(os.environ.get("CHROMOSIGHT_HIP_GATHER_CAP", 0))
        if not slot:
            # the first exchange of this width: every rank must pass the SAME slot (the blocks of a collective have one size), and
            # only the counts of all ranks can say which -- the two-collective form learns them
            out, counts = self.allgather_rows(rows)
            longest = int(counts.max())
            slots[width] = max(longest + longest // 4 + 16, 256)
            return out, counts
        while True:
            out = np.empty((slot * self.world, width))
            rc = self.lib.cs_comm_allgather_rows_once(self.handle, rows.ctypes.data, rows.shape[0], width, slot, out.ctypes.data,
                                                      slot * self.world, counts.ctypes.data)
            longest = int(counts.max()) if self.world else 0
            if rc == -4:                      # CS_ERR_OVERFLOW, on every rank alike: the counts say what slot is needed
                slot = longest + longest // 4 + 16
                continue
            self._check(rc)
            slots[width] = max(longest + longest // 4 + 16, 256)
            return out[:int(counts.sum())], counts

    def allreduce_sum(self, array):
        out = np.ascontiguousarray(array, dtype=np.float64).copy()
        self._check(self.lib.cs_comm_allreduce_f64(self.handle, out.ctypes.data, out.size))
        return out

    def close(self):
        if self.handle:
            self.lib.cs_comm_destroy(self.handle)
            self.handle = None


def native_comm():
    """The RCCL communicator of this process group when the ranks are GPU ranks (torch backend "nccl"), else None (CPU
    tests over gloo keep the torch path).  The 128-byte id is created on rank 0 and broadcast through torch.distributed
    once; every exchange after that goes through the library."""
    dist, rank, world = _world()
    if dist is None or world == 1 or dist.get_backend() != "nccl" or os.environ.get("CHROMOSIGHT_HIP_TORCH_EXCHANGE"):
        return None
    key = (rank, world)
    if key not in _COMMS:
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())

        def all_ok(ok):
            # every rank takes the same branch: a rank that could not load or create its communicator must not leave the
            # others inside a collective of the library
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            return bool(flag.item())

        # 1. local: the library and the RCCL of its HIP runtime load on this rank; rank 0 makes the id
        try:
            from ._lib import load_library
            if load_library().cs_comm_available() != 0:
                raise RuntimeError("librccl of the library's HIP runtime does not load")
            my_id, err = (NativeComm.unique_id() if rank == 0 else None), None
        except Exception as exc:                              # noqa: BLE001 -- whatever it is, the torch path remains
            my_id, err = None, exc
        if not all_ok(err is None):
            _COMMS[key] = None
            if err is not None:
                sys.stderr.write(f"[chromosight_amd] rank {rank}: native RCCL exchange unavailable ({err}); torch.distributed instead\n")
            return None
        box = [my_id if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        # 2. collective: ncclCommInitRank on every rank
        try:
            comm, err = NativeComm(torch.cuda.current_device(), rank, world, box[0]), None
        except Exception as exc:                              # noqa: BLE001
            comm, err = None, exc
        if not all_ok(err is None):
            if comm is not None:
                comm.close()
            comm = None
            if err is not None:
                sys.stderr.write(f"[chromosight_amd] rank {rank}: RCCL communicator not created ({err}); torch.distributed instead\n")
        _COMMS[key] = comm
    return _COMMS[key]


# > 0 while a caller that asked for a purely local run is inside the genome drivers (genome_step(local=True): pipeline.detect):
# an initialised process group is then none of their business -- no sharding of the blocks, no collective
_LOCAL_DEPTH = [0]


def _world():
    if _LOCAL_DEPTH[0] > 0:
        return None, 0, 1
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist, dist.get_rank(), dist.get_world_size()
    except ImportError:
        pass
    return None, 0, 1


def gather_records(records, device=None):
    """All-gather variable-length float64 record arrays (n_i x n_fields) from every rank.
    Count exchange followed by one padded all_gather (fixed-size records)."""
    dist, rank, world = _world()
    records = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, len(RECORD_FIELDS))
    if dist is None or world == 1:
        return records
    comm = native_comm()
    if comm is not None:
        merged, _ = comm.allgather_rows(records)
        return merged[np.argsort(merged[:, 0], kind="stable")]
    import torch
    dev = device if device is not None else (
        torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu"))
    count = torch.tensor([records.shape[0]], dtype=torch.int64, device=dev)
    counts = [torch.zeros_like(count) for _ in range(world)]
    dist.all_gather(counts, count)
    counts = [int(c.item()) for c in counts]
    width = max(max(counts), 1)
    padded = torch.zeros((width, len(RECORD_FIELDS)), dtype=torch.float64, device=dev)
    if records.shape[0]:
        padded[:records.shape[0]] = torch.from_numpy(records).to(dev)
    parts = [torch.zeros_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded)
    out = [p[:c].cpu().numpy() for p, c in zip(parts, counts)]
    merged = np.concatenate(out, axis=0) if out else records
    # block order, then the per-block order of pattern_detector (stable)
    return merged[np.argsort(merged[:, 0], kind="stable")]


def detect_blocks(blocks, kernel_config, kernel_matrix, detector=None, full=True, tsvd=None,
                  loader=None, coords=None):
    """Run pattern_detector on this rank's share of `blocks` and gather all tables.

    blocks : list of contact-map-like objects, or of lightweight descriptors when `loader`
        (a callable descriptor -> contact map) is given; every descriptor needs `.shape`,
        `.max_dist`, `.inter` (the contact maps themselves are only built by the owning rank).
    coords : optional list (one entry per block, or None) of coordinate arrays -> quantify mode.
    Returns a float64 array of records (block, bin1, bin2, score, pvalue), identical on all ranks.
    """
    if detector is None:
        from .utils.detection import pattern_detector as detector
    dist, rank, world = _world()
    costs = []
    for b in blocks:
        shape = b.shape if hasattr(b, "shape") and not hasattr(b, "matrix") else b.matrix.shape
        costs.append(block_cost(shape, b.max_dist, b.inter))
    mine = assign_blocks(costs, world)[rank]
    rows = []
    for idx in mine:
        cmap = loader(blocks[idx]) if loader is not None else blocks[idx]
        block_coords = None if coords is None else coords[idx]
        if coords is not None and block_coords is None:
            continue
        table, _ = detector(cmap, kernel_config, kernel_matrix, coords=block_coords, full=full, tsvd=tsvd)
        if table is None or len(table) == 0:
            continue
        rec = np.empty((len(table), len(RECORD_FIELDS)))
        rec[:, 0] = idx
        rec[:, 1] = table["bin1"].to_numpy(dtype=np.float64)
        rec[:, 2] = table["bin2"].to_numpy(dtype=np.float64)
        rec[:, 3] = table["score"].to_numpy(dtype=np.float64)
        rec[:, 4] = table["pvalue"].to_numpy(dtype=np.float64)
        rows.append(rec)
    local = np.concatenate(rows, axis=0) if rows else np.zeros((0, len(RECORD_FIELDS)))
    return gather_records(local)


# ================================================================================================
# whole-genome detect, blocks sharded over the ranks
# ================================================================================================
GENOME_FIELDS = ("block", "bin1", "bin2", "score", "pvalue", "kernel_id", "iteration")


def _allreduce_sum(array):
    dist, rank, world = _world()
    if dist is None or world == 1:
        return array
    comm = native_comm()
    if comm is not None:
        return comm.allreduce_sum(array).reshape(np.shape(array))
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    t = torch.from_numpy(np.array(array, dtype=np.float64, order="C")).to(dev)     # (a copy: on CPU ranks `.to` shares the caller's memory)
    dist.all_reduce(t)
    return t.cpu().numpy()


def all_gather_rows(array):
    """Rank-order concatenation of every rank's float64 (n_i, w) array, on every rank (count exchange +
    one padded all_gather).  Rows keep their order within a rank."""
    dist, rank, world = _world()
    array = np.ascontiguousarray(array, dtype=np.float64)
    if array.ndim != 2:
        raise ValueError("all_gather_rows needs a 2-D array")
    if dist is None or world == 1:
        return array
    comm = native_comm()
    if comm is not None:
        return comm.allgather_rows(array)[0]
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    count = torch.tensor([array.shape[0]], dtype=torch.int64, device=dev)
    counts = [torch.zeros_like(count) for _ in range(world)]
    dist.all_gather(counts, count)
    counts = [int(c.item()) for c in counts]
    padded = torch.zeros((max(max(counts), 1), array.shape[1]), dtype=torch.float64, device=dev)
    if array.shape[0]:
        padded[:array.shape[0]] = torch.from_numpy(array).to(dev)
    parts = [torch.zeros_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded)
    return np.concatenate([p[:c].cpu().numpy() for p, c in zip(parts, counts)], axis=0)


def split_rows(n, world):
    """Row windows of one n-row block over `world` ranks (equal rows: the band has the same number of
    scanned pixels on every row)."""
    return [(n * r // world, n * (r + 1) // world) for r in range(world)]


def detect_split_block(genome, ci, kernel_config, kernel, tsvd=None, smooth=False, band_dtype=np.float64,
                       want_windows=True, raw=False, staged=None):
    """One intra-chromosomal block over ALL ranks (the single-block case, e.g. one
    200 000-bin chromosome): every rank stages its row window of the block and the template's halo from
    its copy of the pixel table -- no halo exchange --, the per-diagonal (sum, count) of the distance
    law are all-reduced so every part is detrended by the same law, the thresholded pixels are
    all-gathered and labelled identically everywhere, each rank scores the foci of its rows, and the
    records are gathered.  Same (table, windows) as pipeline.detect_block on one GPU, on every rank.
    `staged`: the block returned by an earlier call's stage_split (reused across templates)."""
    from . import pipeline
    block = staged if staged is not None else stage_split(genome, ci, kernel_config, smooth=smooth, band_dtype=band_dtype)
    return pipeline.detect_block(genome, block, kernel_config, kernel, tsvd=tsvd, want_windows=want_windows, raw=raw,
                                 all_gather=all_gather_rows)


def stage_split(genome, ci, kernel_config, smooth=False, band_dtype=np.float64, resident=True):
    """This rank's row window of block `ci`, detrended by the all-reduced distance law."""
    dist, rank, world = _world()
    max_dist = max(kernel_config["max_dist"] // genome.binsize, 1)
    largest = max(np.shape(k)[0] for k in kernel_config["kernels"])
    rows = split_rows(genome.chrom_size(ci), world)[rank]
    if world == 1:
        return genome.stage_intra(ci, max_dist, largest, smooth=smooth, band_dtype=band_dtype, resident=resident)
    return genome.stage_intra(ci, max_dist, largest, smooth=smooth, band_dtype=band_dtype, resident=resident, rows=rows,
                              reduce=_allreduce_sum)


class SplitBlockScan:
    """The correlation pass of ONE sub-matrix row-split over all ranks (the single 200 000-bin block of the
    north star), at map level: rank r owns the output rows split_rows(n, world)[r] and holds only those rows of the band plus
    the template's halo (cs_matrix.row0: no halo exchange).  One step is what the split costs a rank beside its share of
    the tiles:

      1. the per-diagonal (sum, count) of the distance law of its rows all-reduced -- every part must be detrended by the
         same law (stage_split does this once per staging; here it is part of every step so that the collective is timed);
      2. `correlate()`: the coefficient map of its rows (engine.run_normxcorr2(..., row_window=rows));
      3. `candidates()`: the (row, col, value) triples of its rows at or above the threshold, all-gathered so that every
         rank can label the same merged list (detect_split_block continues from there).

    correlate / candidates are the caller's closures (device calls in bench.py and the GPU tests, numpy stand-ins in the CPU
    test); with one rank the step is the correlation call alone -- the exchanges fall away, which makes the 1-rank figure
    the plain kernel figure.  Times of the last step: `exchange_ms` (both collectives), `step_ms`."""

    def __init__(self, n, law_part, correlate, candidates):
        dist, self.rank, self.world = _world()
        self.n = int(n)
        self.rows = split_rows(self.n, self.world)[self.rank]
        self.law_part = np.ascontiguousarray(law_part, dtype=np.float64)
        self.correlate, self.candidates = correlate, candidates
        self.exchange_ms = self.step_ms = 0.0

    def step(self):
        import time
        t0 = time.perf_counter()
        if self.world == 1:
            self.correlate()
            self.step_ms = (time.perf_counter() - t0) * 1e3
            return self.law_part, None
        law = _allreduce_sum(self.law_part)
        t1 = time.perf_counter()
        self.correlate()
        cand = np.ascontiguousarray(self.candidates(), dtype=np.float64).reshape(-1, 3)
        t2 = time.perf_counter()
        merged = all_gather_rows(cand)
        t3 = time.perf_counter()
        self.exchange_ms = ((t1 - t0) + (t3 - t2)) * 1e3
        self.step_ms = (t3 - t0) * 1e3
        return law, merged


def _gather(records, n_fields, once=False):
    """gather_records for an arbitrary record width.  once: the one-collective form of the native exchange (repeating steps)."""
    dist, rank, world = _world()
    records = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, n_fields)
    if dist is None or world == 1:
        return records
    comm = native_comm()
    if comm is not None:
        merged, _ = comm.allgather_rows_once(records) if once else comm.allgather_rows(records)
        return merged[np.argsort(merged[:, 0], kind="stable")]
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    count = torch.tensor([records.shape[0]], dtype=torch.int64, device=dev)
    counts = [torch.zeros_like(count) for _ in range(world)]
    dist.all_gather(counts, count)
    counts = torch.cat(counts).cpu().tolist()                 # one device -> host copy, not one per rank
    width = max(max(counts), 1)
    padded = torch.zeros((width, n_fields), dtype=torch.float64, device=dev)
    if records.shape[0]:
        padded[:records.shape[0]] = torch.from_numpy(records).to(dev)
    parts = [torch.zeros_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded)
    parts = torch.stack(parts).cpu().numpy()                   # likewise
    merged = np.concatenate([parts[r, :c] for r, c in enumerate(counts)], axis=0)
    return merged[np.argsort(merged[:, 0], kind="stable")]


def _own_blocks(genome, kernel_configs, owned=None):
    """This rank's blocks: `owned` when the caller fixed the assignment, else longest-processing-time-first by the pixels scanned
    at the longest keep distance of `kernel_configs`, the same lists on every rank."""
    if owned is not None:
        return list(owned)
    dist, rank, world = _world()
    max_dist = max(max(cfg["max_dist"] // genome.binsize, 1) for cfg in kernel_configs)
    costs = [block_cost((genome.chrom_size(ci),) * 2, max_dist, False) for ci in range(genome.n_chrom)]
    return assign_blocks(costs, world)[rank]


def stage_genome(genome, kernel_configs, owned=None, smooth=False, band_dtype=np.float64, lazy64=None):
    """Stage this rank's blocks for several pattern configurations (detect_genome(..., staged=...)): ONCE at the longest
    keep distance any of them needs, the others scan band views of the same blocks (DeviceCool.view_for).
    lazy64 (default: on for templates of up to 17 x 17 in float32 arithmetic, CHROMOSIGHT_HIP_F64_TWIN=1 turns it off): the
    float64 bands are not stored beyond their first diagonals -- the exact evaluation of the candidates and the windows of
    the records recompute the pixels they read from the pixel table (pipeline.DeviceCool._stage_fast).
    Returns a StagedSet {chromosome: StagedBlock} (for_config(i): the set configuration i scans)."""
    if lazy64 is None:
        from .engine import get_precision
        lazy64 = (not os.environ.get("CHROMOSIGHT_HIP_F64_TWIN") and get_precision() == "f32"
                  and np.dtype(band_dtype) == np.float64
                  and all(max(np.shape(k)) <= 17 for cfg in kernel_configs for k in cfg["kernels"]))
    dists = [max(cfg["max_dist"] // genome.binsize, 1) for cfg in kernel_configs]
    tallest = [max(np.shape(k)[0] for k in cfg["kernels"]) for cfg in kernel_configs]
    owned = _own_blocks(genome, kernel_configs, owned)
    events = hasattr(genome, "dev") and hasattr(genome.dev, "new_event")

    def stage(which, slot):
        md = max(dists[i] for i in which)
        extra = dict(lazy64=True) if lazy64 and hasattr(genome, "_stage_fast") else {}
        out = StagedSet(zip(owned, genome.stage_blocks(owned, md, max(tallest[i] for i in which), smooth=smooth, band_dtype=band_dtype,
                                                       **extra)))
        if events:
            # staging is asynchronous on the genome's stream: streams of other contexts wait for this event, not the host
            name = f"_ready_event{slot}"
            if getattr(genome, name, None) is None:
                setattr(genome, name, genome.dev.new_event())
            genome.dev.record(getattr(genome, name))
            out.ready = getattr(genome, name)
        return out

    wide = list(range(len(kernel_configs)))
    staged = stage(wide, 0)
    staged.by_config = {}
    # Blocks a configuration cannot take as a band view of the shared staging -- a short chromosome staged dense for the
    # widest pattern is a band for a narrower one -- are staged for it here, on the genome's stream, instead of by the
    # host thread that will scan that configuration (detect_patterns: the thread would have to use the genome's context
    # beside the calling thread, and the templates of a 1-D pattern could not share one launch chain).
    # smooth: a fitted law depends on how many diagonals were fitted, so NO block is a view at another keep distance
    # (view_for refuses) -- every configuration with a keep distance of its own gets its blocks staged here, one native call.
    if hasattr(genome, "view_for"):
        extra_any = False
        for i in wide:
            need = []
            for ci in owned:
                blk = staged[ci]
                same = blk.max_dist == dists[i] and blk.keep == min(dists[i], genome.chrom_size(ci)) + tallest[i]
                if not same and genome.view_for(blk, dists[i], tallest[i]) is None:
                    need.append(ci)
            if need:
                own = StagedSet(staged)
                own.update(zip(need, genome.stage_blocks(need, dists[i], tallest[i], smooth=smooth, band_dtype=band_dtype)))
                staged.by_config[i] = own
                extra_any = True
        if extra_any and events:
            genome.dev.record(staged.ready)                  # (one event: after everything staged here)
            for own in staged.by_config.values():
                if own is not None:
                    own.ready = staged.ready
    return staged


class StagedSet(dict):
    """{chromosome: StagedBlock} of stage_genome + the event that fires when their staging is complete."""
    ready = None
    by_config = None

    def for_config(self, i):
        return (self.by_config or {}).get(i) or self


# wall time this process has spent inside record exchanges (bench.py --gpus N reports it per rank)
TIMERS = {"exchange_ms": 0.0, "exchanges": 0}


def _exchange_records(local, n_kernels, n_iterations):
    """The ONE record exchange of a detect call: count + padded all-gather (RCCL: csrc/cs_comm.cpp); per (template,
    iteration) the rows come in the order separate gathers would give -- ranks concatenated, stable by block."""
    if _world()[2] == 1:
        return local                                         # already (template, iteration, block)-ordered
    import time
    t0 = time.perf_counter()
    merged = _gather(local, len(GENOME_FIELDS))              # ranks concatenated, stably sorted by block
    TIMERS["exchange_ms"] += (time.perf_counter() - t0) * 1e3
    TIMERS["exchanges"] += 1
    return merged[np.argsort(merged[:, 5] * n_iterations + merged[:, 6], kind="stable")]


def _exchange_records_many(locals_, kernel_configs):
    """The record exchanges of SEVERAL configurations of one step as ONE exchange (and, on the native transport, one collective:
    NativeComm.allgather_rows_once): the lists travel side by side with the configuration's index in an eighth column and come
    apart again in the order _exchange_records gives each of them."""
    if _world()[2] == 1:
        return list(locals_)
    import time
    t0 = time.perf_counter()
    w = len(GENOME_FIELDS)
    parts = []
    for i, rec in enumerate(locals_):
        rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, w)
        parts.append(np.concatenate([rec, np.full((rec.shape[0], 1), float(i))], axis=1))
    merged = _gather(np.concatenate(parts, axis=0) if parts else np.zeros((0, w + 1)), w + 1, once=True)
    TIMERS["exchange_ms"] += (time.perf_counter() - t0) * 1e3
    TIMERS["exchanges"] += 1
    out = []
    for i, cfg in enumerate(kernel_configs):
        mine = merged[merged[:, w] == i][:, :w]               # (ranks concatenated, stably sorted by block: _gather)
        out.append(mine[np.argsort(mine[:, 5] * cfg["max_iterations"] + mine[:, 6], kind="stable")])
    return out


def transport():
    """What carries this process group's exchanges: "native_rccl" (csrc/cs_comm.cpp), "torch_nccl", "torch_gloo" or "none"."""
    dist, rank, world = _world()
    if dist is None or world == 1:
        return "none"
    if native_comm() is not None:
        return "native_rccl"
    return "torch_" + str(dist.get_backend())


def exchange_self_check():
    """Before a timed multi-GPU region: one padded all-gather of rows with UNEVEN counts (rank r sends 3 r + 1 rows; rank 0
    with a first capacity that is too small, so the retry runs), three exchanges of the one-collective form (slot learnt, slot
    kept, slot outgrown) and one all-reduce through the library's communicator,
    compared with torch.distributed's collectives on the same data.  On a mismatch or an error on ANY rank every rank
    drops to the torch transport, loudly.  Returns the transport in use afterwards."""
    dist, rank, world = _world()
    if dist is None or world == 1:
        return "none"
    comm = native_comm()
    if comm is None:
        return transport()
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    # torch's reference collective first and OUTSIDE the try: every rank issues the same torch collectives whatever happens to
    # the native ones on it (a rank that skipped this all-reduce after a native error would leave the others inside it)
    vec = np.linspace(0.0, 1.0, 97) * (rank + 1)
    t = torch.from_numpy(vec.copy()).to(dev)
    dist.all_reduce(t)
    want_sum = t.cpu().numpy()
    ok, why = True, ""
    try:
        mine = (np.arange((3 * rank + 1) * 5, dtype=np.float64).reshape(-1, 5) + 1000.0 * rank)
        got, counts = comm.allgather_rows(mine, first_cap=2 if rank == 0 else 0)      # (rank 0 too small: the retry runs)
        want = np.concatenate([np.arange((3 * r + 1) * 5, dtype=np.float64).reshape(-1, 5) + 1000.0 * r for r in range(world)])
        if counts.tolist() != [3 * r + 1 for r in range(world)] or not np.array_equal(got, want):
            ok, why = False, "all-gather of rows differs from the expected concatenation"
        # the one-collective form a replayed step uses (cs_comm_allgather_rows_once), on a width of its own: the first exchange learns
        # the slot (two collectives), the second fits it, the third outgrows it on the last rank (every rank sends again)
        for k, grow in enumerate((1, 1, 40)):
            n_r = lambda r: (2 * r + 3) * (grow if r == world - 1 else 1)      # noqa: E731
            mine9 = np.arange(n_r(rank) * 9, dtype=np.float64).reshape(-1, 9) + 1e6 * rank + k
            got9, counts9 = comm.allgather_rows_once(mine9)
            want9 = np.concatenate([np.arange(n_r(r) * 9, dtype=np.float64).reshape(-1, 9) + 1e6 * r + k for r in range(world)])
            if ok and (counts9.tolist() != [n_r(r) for r in range(world)] or not np.array_equal(got9, want9)):
                ok, why = False, f"one-collective all-gather of rows (exchange {k}) differs from the expected concatenation"
        comm.__dict__.get("_slots", {}).pop(9, None)
        got_sum = comm.allreduce_sum(vec)              # (always issued: the native collectives stay matched across the ranks)
        if ok and not np.allclose(got_sum, want_sum, rtol=1e-13, atol=0):
            ok, why = False, "all-reduce differs from torch.distributed's"
    except Exception as exc:                                  # noqa: BLE001 -- whatever it is, the torch path remains
        ok, why = False, repr(exc)
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if not bool(flag.item()):
        if not ok:
            sys.stderr.write(f"[chromosight_amd] rank {rank}: native RCCL exchange failed its self-check ({why}); torch.distributed instead\n")
        _COMMS[(rank, world)] = None
    return transport()


_PATTERN_THREADS = None


def detect_patterns(genome, kernel_configs, owned=None, staged=None, tsvd=None, exchange=True, smooth=False):
    """detect_genome for SEVERAL pattern configurations on blocks staged once (stage_genome), concurrently: a genome
    scan is a few bandwidth / matrix-core-bound launches (a 2-D pattern's tile kernels) next to many latency-bound ones
    (1-D patterns: a few thousand pixels per block and template; labelling, statistics, synchronisations) -- run one after
    the other the latter leave the chip idle, run side by side they disappear under the former.  One host thread per
    configuration whose templates are not iterated; the record exchanges then follow in configuration order on this
    thread (collectives must be issued in the same order on every rank), and so do iterated configurations as a whole.
    smooth: --smooth-trend -- `staged` was staged with it (stage_genome(smooth=True)), and so is whatever a scan stages itself.
    Returns the list of detect_genome results."""
    global _PATTERN_THREADS
    if staged is None:
        staged = stage_genome(genome, kernel_configs, owned=owned, smooth=smooth)
    owned = _own_blocks(genome, kernel_configs, owned)
    complete = all(ci in staged for ci in owned)
    side = [i for i, cfg in enumerate(kernel_configs) if cfg["max_iterations"] == 1] if complete and len(kernel_configs) > 1 else []
    if _PATTERN_THREADS is None and side:
        import concurrent.futures
        _PATTERN_THREADS = concurrent.futures.ThreadPoolExecutor(max_workers=4, thread_name_prefix="chromosight-pattern")
    ready = getattr(staged, "ready", None)
    if side and ready is None:
        genome.dev.sync()                                    # staging is complete before several threads and streams read it
    pick = lambda i: staged.for_config(i) if isinstance(staged, StagedSet) else staged
    # the configuration that scans the widest band stays on this thread (a hand-over to a pool thread costs 50-100 us, and
    # its pass is the longest); the others go to the pool first
    here = max(side, key=lambda i: kernel_configs[i]["max_dist"]) if side else None
    futures = {i: _PATTERN_THREADS.submit(detect_genome, genome, kernel_configs[i], tsvd=tsvd, owned=owned, staged=pick(i), smooth=smooth,
                                          exchange=False, exclusive=len(side) < 2, own_context=True)
               for i in side if i != here}
    local = {}
    if here is not None:
        local[here] = detect_genome(genome, kernel_configs[here], tsvd=tsvd, owned=owned, staged=pick(here), smooth=smooth, exchange=False,
                                    exclusive=len(side) < 2)
    results = [None] * len(kernel_configs)
    for i, cfg in enumerate(kernel_configs):
        if i not in side:
            results[i] = detect_genome(genome, cfg, tsvd=tsvd, owned=owned, staged=pick(i), smooth=smooth, exclusive=not side, exchange=exchange)
    for i in side:                                           # (collectives in the same order on every rank)
        mine = local[i] if i in local else futures[i].result()
        # (exchange=False: this rank's records -- genome_step exchanges the configurations of a step together)
        results[i] = _exchange_records(mine, len(kernel_configs[i]["kernels"]), 1) if exchange else mine
    return results


def genome_step(genome, kernel_configs, owned=None, tsvd=None, local=False, smooth=False):
    """One detect step of a sharded genome: stage_genome + detect_patterns, the results of detect_patterns.
    local=True: this process alone, whatever process group is initialised -- every block, no collective (pipeline.detect: a
    call one rank may make on its own, as the reference's detect is).  For the usual
    pair of configurations (a 2-D pattern and a 1-D pattern with several templates, single iterations) every step after the
    first is ONE native call on the arguments the first step used (chromosight_amd/plan.py: cs_run_calls) plus one record
    exchange per configuration; anything else -- and any step whose call list reports an error -- takes the two calls.
    smooth: --smooth-trend (the laws fitted on the device by the staging call; a step of its own plan)."""
    if local:
        _LOCAL_DEPTH[0] += 1
        try:
            return genome_step(genome, kernel_configs, owned=owned, tsvd=tsvd, smooth=smooth)
        finally:
            _LOCAL_DEPTH[0] -= 1
    from . import plan as _plan
    owned = _own_blocks(genome, kernel_configs, owned)
    if not owned or not _plan.plannable(genome, kernel_configs, tsvd, smooth=smooth):
        staged = stage_genome(genome, kernel_configs, owned=owned, smooth=smooth)
        return detect_patterns(genome, kernel_configs, owned=owned, staged=staged, tsvd=tsvd, smooth=smooth)
    key = (tuple(owned), bool(smooth), tuple((cfg["max_dist"], cfg["pearson"], cfg["max_perc_undetected"], cfg["max_perc_zero"],
                                tuple(np.asarray(k, dtype=np.float64).tobytes() for k in cfg["kernels"])) for cfg in kernel_configs))
    plans = genome.__dict__.setdefault("_step_plans", {})
    plan = plans.get(key)
    if plan is not None and plan.ok:
        local = plan.run()
        if local is not None:
            return _exchange_records_many(local, kernel_configs)     # (one exchange for the step's configurations)
        plans.pop(key, None)                                  # (a result list outgrew its capacity: the usual path, a new plan)
    from . import _lib
    _lib.CAPTURE = captured = []
    try:
        staged = stage_genome(genome, kernel_configs, owned=owned, smooth=smooth)
        # (this rank's records, then the ONE exchange a replayed step makes too: whichever way a rank takes through a step --
        # a plan that outgrew its buffers falls back here -- the ranks issue the same collectives)
        results = detect_patterns(genome, kernel_configs, owned=owned, staged=staged, tsvd=tsvd, exchange=False, smooth=smooth)
    finally:
        _lib.CAPTURE = None
    results = _exchange_records_many(results, kernel_configs)
    if len(plans) > 8:
        plans.clear()
    plans[key] = _plan.StepPlan(genome, kernel_configs, owned, captured, staged)
    return results


def _device_pileup(genome, staged, local, kernel_shape, dev=None, stream=None):
    """(sum, count) over the windows of this rank's records `local` (GENOME_FIELDS rows: block, block-local bin1, bin2, ...) of
    one template and iteration, from the staged blocks they were detected on (pipeline.pileup_blocks); zeros without records."""
    if local.shape[0] == 0:
        return np.zeros(kernel_shape), np.zeros(kernel_shape, dtype=np.int64)
    from . import pipeline
    ids, blk = np.unique(local[:, 0].astype(np.int64), return_inverse=True)
    return pipeline.pileup_blocks(genome, [staged[int(ci)] for ci in ids], kernel_shape, blk, local[:, 1], local[:, 2], dev=dev, stream=stream)


def _records(block_ids, table, kernel_id, iteration):
    """GENOME_FIELDS rows of one template and iteration.  block_ids: one block's index (the table of that block) or one index per
    row (a table merged over blocks); table: a (k, 4) array (bin1, bin2, score, pvalue) or a DataFrame with these columns."""
    rec = np.empty((len(table), len(GENOME_FIELDS)))
    rec[:, 0] = block_ids
    rec[:, 1:5] = table if isinstance(table, np.ndarray) else table[["bin1", "bin2", "score", "pvalue"]].to_numpy(dtype=np.float64)
    rec[:, 5] = kernel_id
    rec[:, 6] = iteration
    return rec


def _refine(total, count, n_records):
    """The template an iterated pattern continues with (cli/chromosight.py:791): the pileup sum / count over the windows of ALL
    ranks, from this rank's (sum, count) per template pixel and its number of records -- or None when no rank found a pattern
    (next template, cli/chromosight.py:786-789).  With several ranks ONE all-reduce carries the three together (2 km kn + 1
    doubles).  0 / 0 is NaN, as in np.nanmean (detection.py:158-174)."""
    both = _allreduce_sum(np.concatenate([np.ravel(total), np.ravel(count).astype(np.float64), [float(n_records)]]))
    if both[-1] == 0:
        return None
    kk = np.size(total)
    with np.errstate(all="ignore"):
        return (both[:kk] / both[kk:2 * kk]).reshape(np.shape(total))


def detect_genome(genome, kernel_config, tsvd=None, smooth=False, band_dtype=np.float64, stage=None, detect=None,
                  owned=None, staged=None, exchange=True, exclusive=True, own_context=False):
    """`chromosight detect` over all intra-chromosomal blocks of a DeviceCool, sharded over the ranks
    like the reference's Pool.imap over sub-matrices (cli/chromosight.py:738-755): every rank stages
    and scans its own blocks (LPT assignment by band pixels), the records of all templates and iterations
    are all-gathered ONCE at the end (count + padded all_gather: RCCL over xGMI with the "nccl" backend),
    and when the template is refined over iterations every non-final iteration ends with _refine: one all-reduce
    of the per-rank pileup sums, counts and record numbers, so every rank continues with the same template.

    How a template is scanned is chosen once, before the template x iteration loop: block by block through the
    injected `stage` / `detect`; else -- the device pipeline -- the templates of a 1-D pattern in one launch chain on a
    worker context (pipeline.detect_blocks_templates), several single-iteration templates side by side on worker
    contexts, a template on this thread's own worker context (own_context), or the batched call on the genome's context.

    `genome` needs n_chrom, chrom_size(ci), binsize; `stage(genome, ci, max_dist, largest)` and
    `detect(genome, block, cfg, kernel, tsvd)` default to the device pipeline (injected in CPU tests).
    `owned`: this rank's block indices when the caller fixed the assignment (e.g. a rank that only
    holds the pixels of its own chromosomes); default: LPT by scanned pixels.
    `staged`: blocks of stage_genome (staged once for several patterns); a block that cannot serve this configuration
    through a band view is staged here as usual.  exchange=False: this rank's records only (detect_patterns).
    exclusive=False: other configurations are being scanned on this GPU at the same time (detect_patterns).
    own_context=True: this call runs on a host thread beside another one that uses the genome's own context and stream
    (detect_patterns): every device call goes to a context and stream of this thread (a context serves one call in flight).
    Returns float64 records (block, bin1, bin2, score, pvalue, kernel_id, iteration), block-local
    bins, identical on all ranks, in the single-process order."""
    device_route = stage is None and detect is None          # the device pipeline stages and scans: nothing is injected
    if stage is None or detect is None:
        from . import pipeline
        stage = stage or (lambda g, ci, md, lk: g.stage_intra(ci, md, lk, smooth=smooth, band_dtype=band_dtype,
                                                              resident=True))
        detect = detect or (lambda g, blk, cfg, k, t: pipeline.detect_block(g, blk, cfg, k, tsvd=t, raw=True))
    kernels = [np.asarray(k, dtype=np.float64) for k in kernel_config["kernels"]]
    n_iter = kernel_config["max_iterations"]
    max_dist = max(kernel_config["max_dist"] // genome.binsize, 1)
    largest = max(np.shape(k)[0] for k in kernels)
    mine = _own_blocks(genome, [kernel_config], owned)
    have = {}
    if staged is not None:
        for ci in mine:
            blk = staged.get(ci)
            # (a block staged with the other kind of law is not this call's block; a smoothed one serves its own keep
            # distance only: view_for refuses it)
            if blk is None or blk.smooth != bool(smooth):
                continue
            view = blk if (blk.max_dist == max_dist and blk.keep == min(max_dist, genome.chrom_size(ci)) + largest) \
                else genome.view_for(blk, max_dist, largest)
            if view is not None:
                have[ci] = view
    todo = [ci for ci in mine if ci not in have]
    # the event of the caller's staging; it does not cover blocks staged here
    ready = getattr(staged, "ready", None) if not todo else None
    if device_route:
        # the device pipeline stages its blocks with one native call (pipeline.DeviceCool.stage_blocks)
        fresh = dict(zip(todo, genome.stage_blocks(todo, max_dist, largest, smooth=smooth, band_dtype=band_dtype))) if todo else {}
    else:
        fresh = {ci: stage(genome, ci, max_dist, largest) for ci in todo}
    staged = {**have, **fresh}
    blocks = [staged[ci] for ci in mine]

    def batch(kernel, want_windows, defer=False, dev=None, stream=None):
        return pipeline.detect_blocks(genome, blocks, kernel_config, kernel, tsvd=tsvd, raw=True, want_windows=want_windows, defer=defer,
                                      dev=dev, stream=stream, merged=True, exclusive=exclusive and len(kernels) == 1)

    def after_staging(pool):
        """On the calling thread: the host waits for the genome's stream when no event says that the staged blocks are complete.
        Returns a callable for a thread of `pool`: its (dev, stream), the stream behind that event."""
        if ready is None:
            genome.dev.sync()

        def take():
            dev, stream = pool.device()
            if ready is not None:
                dev.wait_event(ready, stream)                # device-side: the staging of these blocks has finished
            return dev, stream

        return take

    def parts_of(results):
        """What a scan found as ([(block ids, table)], [windows]), from the merged triple of a batch entry (the table of all
        blocks, the records per block, windows or None) or from one (table, windows) per block."""
        if isinstance(results, tuple):
            table, kept, windows = results
            return [(np.repeat(np.asarray(mine, dtype=np.float64), kept), table)], [] if windows is None else [windows]
        found = [(ci, table, windows) for ci, (table, windows) in zip(mine, results) if table is not None and len(table)]
        return [(ci, table) for ci, table, _ in found], [windows for _, _, windows in found if windows is not None]

    # scan(kernel_id, kernel, need_windows): this rank's parts_of for one template.  The route is chosen here, once.
    # Templates that do not depend on each other (a single iteration each) are scanned concurrently when the genome has worker
    # contexts (pipeline._Workers); CHROMOSIGHT_HIP_NO_TEMPLATE_OVERLAP=1 scans them in turn.
    side_by_side = (device_route and n_iter == 1 and bool(mine) and hasattr(genome, "workers")
                    and not os.environ.get("CHROMOSIGHT_HIP_NO_TEMPLATE_OVERLAP"))
    pile_on = (None, None)                                   # where the device pileup runs: the genome's context and stream
    joint = None
    if side_by_side and kernel_config["max_dist"] == 0 and tsvd is None and not todo:
        # a 1-D pattern's templates share one launch chain (cs_detect_foci_batch_templates): on a worker context, so that the
        # chain runs beside whatever this genome's own stream is doing (another pattern's tile kernels).  ONE template --
        # hairpins -- takes it too: the entry serves 1 to 4 templates, and it is the chain a StepPlan replays (plan.py)
        dev, stream = after_staging(genome.workers(1))()
        joint = pipeline.detect_blocks_templates(genome, blocks, kernel_config, kernels, dev=dev, stream=stream)
    if not device_route:
        scan = lambda kernel_id, kernel, need_windows: parts_of([detect(genome, staged[ci], kernel_config, kernel, tsvd) for ci in mine])
    elif joint is not None:
        joint = joint()                                      # the acceptance rules, here
        scan = lambda kernel_id, kernel, need_windows: parts_of(joint[kernel_id])
    elif side_by_side and len(kernels) > 1:
        # one host thread per template, each with its own context and stream on this GPU, so the latency-bound stages of one
        # template's chain (labelling, statistics, the synchronisations) run under another's.  The acceptance rules (many small
        # numpy calls) run in scan, on this thread, one template after the other while the others are on the device: spread
        # over the worker threads they fight for the interpreter lock and each takes four times as long
        pool = genome.workers(min(len(kernels), 3))
        take = after_staging(pool)

        def chain(kernel):
            dev, stream = take()
            return batch(kernel, False, True, dev, stream)

        futures = [pool.pool.submit(chain, kernel) for kernel in kernels]
        scan = lambda kernel_id, kernel, need_windows: parts_of(futures[kernel_id].result()())
    elif own_context and hasattr(genome, "workers"):
        # on a pool thread: not on the genome's context, which the calling thread is using
        pool = genome.workers(1)
        pile_on = pool.device()

        def scan(kernel_id, kernel, need_windows):
            dev, stream = after_staging(pool)()              # (before every call: each one reads the staged blocks)
            return parts_of(batch(kernel, need_windows, False, dev, stream))
    else:
        scan = lambda kernel_id, kernel, need_windows: parts_of(batch(kernel, need_windows))
    # An iterated template's pileup is reduced where its windows are (pipeline.pileup_blocks: the accepted records' pixels of the
    # staged blocks, 2 km kn numbers back) when the device pipeline is in use: no iteration fetches windows then.
    # CHROMOSIGHT_HIP_HOST_PILEUP=1 (and injected stage / detect): the windows of the non-final iterations are fetched and
    # summed on the host.
    device_pileup = device_route and n_iter > 1 and not pipeline.host_pileup()
    pending = []                                             # gathered once, at the end of the call
    for kernel_id, kernel in enumerate(kernels):
        for it in range(n_iter):
            last = it + 1 == n_iter
            parts, wins = scan(kernel_id, kernel, not last and not device_pileup)
            local = np.concatenate([_records(ids, table, kernel_id, it) for ids, table in parts] or [np.zeros((0, len(GENOME_FIELDS)))])
            pending.append(local)
            if last:
                break                                        # nothing depends on the last iteration's patterns: no windows, no reduction
            if device_pileup:
                total, count = _device_pileup(genome, staged, local, kernel.shape, *pile_on)
            else:
                stack = np.concatenate(wins, axis=0) if wins else np.zeros((0,) + kernel.shape)
                total, count = np.nansum(stack, axis=0), np.sum(~np.isnan(stack), axis=0)
            kernel = _refine(total, count, local.shape[0])
            if kernel is None:
                break
    local = np.concatenate(pending, axis=0) if pending else np.zeros((0, len(GENOME_FIELDS)))
    if not exchange:
        return local                                         # detect_patterns: the caller exchanges (in a fixed order)
    return _exchange_records(local, len(kernels), n_iter)


# ================================================================================================
# `detect --inter`, sub-matrices (intra blocks, trans blocks in strips) sharded over the ranks
# ================================================================================================
def inter_unit_costs(pairs, sizes, max_dist, largest):
    """Pixels of every (ca, cb) unit of `detect --inter` (pipeline.sub_matrices order), from the shapes alone: the band an
    intra block scans, n * min(max_dist + largest, n), and the whole area n_r * n_c of a trans block (its strip fill, the
    occupancy narrowing and the list kernel all scale with the area when few tiles are empty)."""
    sizes = [int(n) for n in sizes]
    return [sizes[a] * min(int(max_dist) + int(largest), sizes[a]) if a == b else sizes[a] * sizes[b] for a, b in pairs]


class DetectShard:
    """How pipeline.detect(inter=True) shares its sub-matrices among the ranks (detect_inter_genome): `select` keeps this
    rank's units -- LPT (assign_blocks) over inter_unit_costs, the same lists on every rank --, `merge` all-gathers the
    per-unit tables (and windows) after every template and iteration, so that every rank continues with the list the single
    process builds: tables and windows of all units in sub_matrices order.

    owned: this rank's unit indices, fixed by the caller (default: LPT).  exchange=False: nothing is merged, every rank keeps
    its own units' tables (a share timed alone); only with single-iteration templates -- the next template of an iteration
    is the pileup of ALL units' windows."""

    def __init__(self, owned=None, exchange=True):
        self.dist, self.rank, self.world = _world()
        self.owned = None if owned is None else sorted(int(u) for u in owned)
        self.exchange = bool(exchange)

    def check(self, kernel_config):
        """Argument checks (pipeline.detect runs them before any device work or collective)."""
        if not self.exchange and kernel_config["max_iterations"] != 1:
            raise ValueError("DetectShard(exchange=False) needs max_iterations == 1: an iteration's template is the pileup of all units")

    def select(self, pairs, sizes, max_dist, largest):
        if self.owned is not None:
            if any(u < 0 or u >= len(pairs) for u in self.owned):
                raise ValueError(f"DetectShard: owned units must be in 0 .. {len(pairs) - 1}")
            return list(self.owned)
        if self.world == 1:
            return list(range(len(pairs)))
        return assign_blocks(inter_unit_costs(pairs, sizes, max_dist, largest), self.world)[self.rank]

    def merge(self, units, results, kernel_shape, need_windows):
        """units: this rank's unit indices; results: their (table (k, 4) or None, windows (k, km, kn) or None).  Returns (unit
        indices, results) of every unit of every rank that found something, in unit order -- ONE count exchange and ONE padded
        all-gather of rows [unit, bin1, bin2, score, pvalue] (+ km * kn window values with need_windows), whatever this rank
        holds."""
        if not self.exchange or self.world == 1:
            return units, results
        kk = int(np.prod(kernel_shape)) if need_windows else 0
        parts = []
        for u, (tab, win) in zip(units, results):
            if tab is None or len(tab) == 0:
                continue
            rec = np.empty((len(tab), 5 + kk))
            rec[:, 0] = u
            rec[:, 1:5] = tab
            if kk:
                rec[:, 5:] = np.asarray(win, dtype=np.float64).reshape(len(tab), kk)
            parts.append(rec)
        local = np.concatenate(parts, axis=0) if parts else np.zeros((0, 5 + kk))
        import time
        t0 = time.perf_counter()
        merged = all_gather_rows(local)
        TIMERS["exchange_ms"] += (time.perf_counter() - t0) * 1e3
        TIMERS["exchanges"] += 1
        # ranks concatenated; every unit comes from ONE rank with its rows in order: a stable sort by unit is the unit order
        merged = merged[np.argsort(merged[:, 0], kind="stable")]
        done, out = [], []
        ids = merged[:, 0].astype(np.int64)
        cuts = np.flatnonzero(np.diff(ids)) + 1
        for rows in np.split(merged, cuts) if merged.shape[0] else []:
            done.append(int(rows[0, 0]))
            win = rows[:, 5:].reshape((rows.shape[0],) + tuple(kernel_shape)) if kk else None
            out.append((np.ascontiguousarray(rows[:, 1:5]), win))
        return done, out


def detect_inter_genome(cool, kernel_config, **options):
    """`chromosight detect --inter` with the sub-matrices sharded over the ranks like the reference's process pool
    (cli/chromosight.py:738-755): every rank stages and scans its own intra blocks and its own trans blocks (in row strips of at
    most inter_budget bytes), the per-unit tables are all-gathered after every template and iteration, and every rank returns
    the table (with return_windows, also the windows) a single process returns.  Options: those of pipeline.detect."""
    from . import pipeline
    return pipeline.detect(cool, kernel_config, inter=True, shard=DetectShard(), **options)


# ================================================================================================
# `quantify`, sub-matrices sharded over the ranks
# ================================================================================================
class QuantifyShard:
    """How pipeline.quantify shares its sub-matrices among the ranks: `select` keeps this rank's share of the (ca, cb,
    positions, coordinates) work list -- longest-processing-time-first by the pixels a sub-matrix stages plus the windows its
    positions read, the same list on every rank --, `merge` exchanges the scores once (one padded all-gather of
    (position, template, score, p-value, window) rows: RCCL with the "nccl" backend, gloo in the CPU tests)."""
    prices_strips = True                      # (pipeline.quantify hands select the strip budget and the template reach)

    def __init__(self):
        self.dist, self.rank, self.world = _world()

    def select(self, todo, dcool, max_dist, budget=None, reach=None):
        """budget, reach: inter_budget and the largest template's side -- a trans sub-matrix is then priced by the rows its strips
        stage (pipeline._row_groups, halo included) times its columns; without them by its whole area."""
        from . import pipeline
        costs = []
        for ca, cb, sel, coords in todo:
            n_r, n_c = dcool.chrom_size(ca), dcool.chrom_size(cb)
            if ca == cb:
                staged = n_r * min(max_dist + 1, n_c)
            elif budget is None or reach is None:
                staged = n_r * n_c
            else:
                halo = (reach - 1) // 2
                rows = np.unique(np.clip(np.asarray(coords, dtype=np.int64).reshape(-1, 2)[:, 0], 0, n_r - 1))
                groups = pipeline._row_groups(rows, n_r, n_c, budget, halo)
                staged = sum(hi - lo for lo, hi in (pipeline._strip_rows(n_r, g, halo) for g in groups)) * n_c
            costs.append(int(staged) + 512 * len(sel))
        owned = assign_blocks(costs, self.world)[self.rank]
        return [todo[i] for i in owned]

    def merge(self, score_out, pval_out, win_out, sels):
        n_k = len(score_out)
        kk = int(np.prod(win_out[0].shape[1:]))
        where = np.concatenate(sels) if sels else np.zeros(0, dtype=np.int64)
        rows = np.empty((n_k * where.size, 4 + kk))
        for k in range(n_k):
            part = rows[k * where.size:(k + 1) * where.size]
            part[:, 0] = where
            part[:, 1] = k
            part[:, 2] = score_out[k][where]
            part[:, 3] = pval_out[k][where]
            part[:, 4:] = win_out[k][where].reshape(where.size, kk)
        merged = all_gather_rows(rows)
        pos = merged[:, 0].astype(np.int64)
        for k in range(n_k):
            m = merged[:, 1] == k
            score_out[k][pos[m]] = merged[m, 2]
            pval_out[k][pos[m]] = merged[m, 3]
            win_out[k][pos[m]] = merged[m, 4:].reshape((-1,) + win_out[k].shape[1:])
        return score_out, pval_out, win_out


def quantify_genome(cool, positions, kernel_config, **options):
    """`chromosight quantify` with the sub-matrices sharded over the ranks like the reference's process pool
    (cli/chromosight.py:396-410: one task per sub-matrix that holds a position): every rank stages and scores its own
    sub-matrices (pipeline.quantify: one native call per template over all of them), ONE exchange carries the scores, and
    every rank returns the same (table, windows) a single process returns."""
    from . import pipeline
    return pipeline.quantify(cool, positions, kernel_config, shard=QuantifyShard(), **options)
