"""Sparse libsvm input path: parser, CSR batches, DataProvider.

Reference (lr2.py): `Sample.parse_line_libsvm` (:57-67) splits each line in
Python; `format_samples_sparse` (:69-84) builds COO `[[row, fid], ...]` lists;
`LoadDataThread` (:87-155) has N Python threads read strided files through
GFile with per-line Bernoulli sampling, either materialising everything
('all') or pushing raw lines into a TF FIFOQueue forever ('queue');
`DataProvider` (:177-304) shards files per worker (`files[task::workers]`),
shuffles per epoch, yields batches and samples a test subset.

Here the parsing is native C++ (csrc/runtime/libsvm.cpp: one thread per file
group, no GIL, sampling in the parser) and a batch is *CSR* --
(labels [B,1] f32, offsets [B+1] i64, ids [nnz] i64, vals [nnz] f32) -- which
is exactly what the embedding-bag kernel consumes; the COO `sp_indices` of the
reference is derivable (`CSRBatch.coo_indices`).  'queue' mode is the native
`LibsvmStream` (bounded queue of ready CSR batches, looping over the files).
Intentional fix: the reference's queue-mode test sampler reads the *train*
queue (lr2.py:213-217, "should be 'test'"); here it reads the test stream.

`parser="gpu"` (opt-in; the default stays "cpu") parses the text on the GPU
instead (csrc/kernels/libsvm_parse.hip): file bytes go through pinned buffers to
the device and come out as `DeviceCSR` -- device CSR already cut into batches,
each a zero-copy view -- which the sparse trainers take as they take a
`CSRBatch.to(device)` tuple.  At sampling rate 1 both parsers give the same
bits (a chunk the GPU's strict grammar does not cover is parsed by the C++
parser instead); at a rate below 1 the GPU path keeps another sample: see
`GpuLibsvmParser`.
"""
from __future__ import annotations

import os
import queue
import threading
import time
from dataclasses import dataclass
from typing import Iterator, List, Optional, Sequence

import numpy as np

from .. import _native
from ..utils import gfile
from ..utils import logging as log


@dataclass
class CSRBatch:
    labels: np.ndarray     # [B, 1] float32
    offsets: np.ndarray    # [B + 1] int64
    ids: np.ndarray        # [nnz] int64
    vals: np.ndarray       # [nnz] float32

    @property
    def size(self) -> int:
        return len(self.offsets) - 1

    @property
    def nnz(self) -> int:
        return len(self.ids)

    def coo_indices(self) -> np.ndarray:
        """[[row, fid], ...] of lr2.py:82-83 (SparseTensor indices)."""
        rows = np.repeat(np.arange(self.size, dtype=np.int64), np.diff(self.offsets))
        return np.stack([rows, self.ids], 1)

    def as_tf_feed(self):
        """(labels, fids, fvals, sp_indices, size) == Sample.format_samples_sparse."""
        return self.labels, self.ids, self.vals, self.coo_indices(), self.size

    def to(self, device):
        import torch

        return (torch.from_numpy(self.labels).to(device, non_blocking=True),
                torch.from_numpy(self.offsets).to(device, non_blocking=True),
                torch.from_numpy(self.ids).to(device, non_blocking=True),
                torch.from_numpy(self.vals).to(device, non_blocking=True))


class CSRData:
    """A materialised CSR sample set with vectorised row gathering."""

    def __init__(self, labels, offsets, ids, vals):
        self.labels = np.asarray(labels, np.float32).reshape(-1)
        self.offsets = np.asarray(offsets, np.int64)
        self.ids = np.asarray(ids, np.int64)
        self.vals = np.asarray(vals, np.float32)

    @staticmethod
    def concat(parts: Sequence["CSRData"]) -> "CSRData":
        parts = [p for p in parts if p is not None and len(p)]
        if not parts:
            return CSRData(np.zeros(0), np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0))
        offs, base = [np.zeros(1, np.int64)], 0
        for p in parts:
            offs.append(p.offsets[1:] + base)
            base += p.offsets[-1]
        return CSRData(np.concatenate([p.labels for p in parts]), np.concatenate(offs),
                       np.concatenate([p.ids for p in parts]), np.concatenate([p.vals for p in parts]))

    def __len__(self):
        return len(self.labels)

    def take(self, rows: np.ndarray) -> CSRBatch:
        rows = np.asarray(rows, np.int64)
        starts, ends = self.offsets[rows], self.offsets[rows + 1]
        lens = ends - starts
        offs = np.zeros(len(rows) + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        idx = np.repeat(starts - offs[:-1], lens) + np.arange(offs[-1], dtype=np.int64)
        return CSRBatch(self.labels[rows].reshape(-1, 1), offs, self.ids[idx], self.vals[idx])

    def slice(self, s: int, e: int) -> CSRBatch:
        return self.take(np.arange(s, e))


def parse_lines(lines: Sequence[str], sampling_rate: float = 1.0, seed: int = 0) -> CSRData:
    data = "".join(l if l.endswith("\n") else l + "\n" for l in lines).encode()
    y, rp, ids, vals = _native.load().libsvm_parse_bytes(data, sampling_rate, seed)
    return CSRData(y, rp, ids, vals)


def load_files(files: Sequence[str], nthreads: int = 2, sampling_rate: float = 1.0, seed: int = 0,
               parser: str = "cpu", device=None) -> CSRData:
    """Parse files (local, file:// or hdfs://) with `nthreads` native threads, or,
    with parser="gpu", on `device` (default: the current GPU) in file order and
    bring the result back to the host.  The GPU result equals the nthreads=1 CPU
    result at sampling_rate 1; below 1 it is the hashed sample (GpuLibsvmParser)."""
    if parser not in ("cpu", "gpu"):
        raise ValueError("parser must be 'cpu' or 'gpu'")
    if parser == "gpu":
        gp = GpuLibsvmParser(device=device, sampling_rate=sampling_rate, seed=seed)
        return CSRData.concat([d.to_host() for d in gp.parse_files(files)])
    C = _native.load()
    local = [gfile.local_path(f) for f in files]
    if all(p is not None for p in local):
        y, rp, ids, vals = C.libsvm_parse_files(list(local), int(nthreads), float(sampling_rate), int(seed))
        return CSRData(y, rp, ids, vals)
    parts = []
    for i, f in enumerate(files):    # remote scheme: stream bytes through GFile
        with gfile.GFile(f, "rb") as fh:
            y, rp, ids, vals = C.libsvm_parse_bytes(fh.read(), float(sampling_rate), int(seed) + i)
        parts.append(CSRData(y, rp, ids, vals))
    return CSRData.concat(parts)


class DeviceCSR:
    """One parsed chunk on the GPU, cut into batches of `batch_size` rows.

    labels [R] f32, ids / vals [nnz], offsets [batches, batch_size + 1] i64 with
    every row rebased on its batch's first entry, bases (host int64
    [batches + 1]) into ids / vals: batch b is views of the four, no copy.
    `carry_rows` > 0 (a stream's chunk): the first batch is short by that many
    rows -- it completes rows carried over from the chunk before -- and its
    offsets continue from `carry_nnz`."""

    def __init__(self, labels, offsets, ids, vals, bases, batch_size, carry_rows=0, carry_nnz=0, lines=0,
                 irregular=False, bad_lines=0):
        self.labels, self.offsets, self.ids, self.vals = labels, offsets, ids, vals
        self.bases = np.asarray(bases, np.int64)
        self.batch_size, self.carry_rows, self.carry_nnz = int(batch_size), int(carry_rows), int(carry_nnz)
        self.lines, self.irregular, self.bad_lines = int(lines), bool(irregular), int(bad_lines)

    def __len__(self):
        return int(self.labels.shape[0])

    @property
    def nnz(self) -> int:
        return int(self.ids.shape[0])

    @property
    def num_batches(self) -> int:
        return int(self.offsets.shape[0])

    def _span(self, b):
        """(first row, end row, first offsets column) of batch b."""
        bs, c, R = self.batch_size, self.carry_rows, len(self)
        return max(b * bs - c, 0), min((b + 1) * bs - c, R), (c if b == 0 else 0)

    def batch(self, b):
        r0, r1, j0 = self._span(b)
        s, e = int(self.bases[b]), int(self.bases[b + 1])
        return (self.labels[r0:r1].view(-1, 1), self.offsets[b, j0:j0 + (r1 - r0) + 1], self.ids[s:e], self.vals[s:e])

    def batches(self):
        """(labels [B,1], offsets [B+1], ids, vals) device views, batch by batch."""
        for b in range(self.num_batches):
            yield self.batch(b)

    def to_host(self) -> CSRData:
        off = self.offsets.cpu().numpy()
        parts = [np.zeros(1, np.int64)]
        for b in range(self.num_batches):
            r0, r1, j0 = self._span(b)
            parts.append(off[b, j0 + 1:j0 + 1 + (r1 - r0)] - off[b, j0] + self.bases[b])
        return CSRData(self.labels.cpu().numpy(), np.concatenate(parts), self.ids.cpu().numpy(),
                       self.vals.cpu().numpy())


def _after_last_newline(buf: np.ndarray, n: int) -> int:
    """One past the last '\\n' of buf[:n], 0 when there is none (searched from the end, 64 KB at a time)."""
    e = n
    while e > 0:
        s = max(0, e - 65536)
        hit = np.flatnonzero(buf[s:e] == 10)
        if hit.size:
            return s + int(hit[-1]) + 1
        e = s
    return 0


class GpuLibsvmParser:
    """libsvm text -> `DeviceCSR` with the HIP parser (native `LibsvmGpuParser`).

    The kernels accept a strict grammar and compute every number so that it
    equals strtof's; a chunk holding anything else (inf, nan, hex floats, signed
    or very long indices, stray bytes, numbers of more than 15 digits or on a
    float32 tie, ...) is parsed by the C++ parser instead and uploaded
    (`fallback_chunks`, `bad_lines`).  So at sampling_rate 1 the result is the
    C++ parser's, bit for bit.  At sampling_rate < 1 the C++ parser draws from a
    sequential xorshift per line, which cannot be evaluated in parallel: this
    parser keeps line `ordinal` -- a running count of the '\\n'-separated pieces
    of the call or the stream -- iff a hash of (seed, ordinal) is below the
    rate: a different, equally distributed, deterministic sample
    (`libsvm_parse_bytes_hashed` is its host form)."""

    def __init__(self, device=None, chunk_bytes: int = 16 << 20, batch_size: int = 500, sampling_rate: float = 1.0,
                 seed: int = 0):
        import torch

        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("GpuLibsvmParser needs a GPU device")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.chunk_bytes, self.batch_size = int(chunk_bytes), int(batch_size)
        self._p = _native.load().LibsvmGpuParser(self.device.index, self.chunk_bytes, self.batch_size,
                                                 float(sampling_rate), int(seed))
        self._stage = [self._p.staging(0).numpy(), self._p.staging(1).numpy()]

    gpu_chunks = property(lambda self: self._p.gpu_chunks)
    fallback_chunks = property(lambda self: self._p.fallback_chunks)
    bad_lines = property(lambda self: self._p.bad_lines)

    def _wrap(self, res, carry_rows, carry_nnz):
        labels, offsets, ids, vals, bases, _rows, _nnz, lines, irregular, bad = res
        return DeviceCSR(labels, offsets, ids, vals, bases.numpy(), self.batch_size, carry_rows, carry_nnz, lines,
                         irregular, bad)

    def parse_bytes(self, data: bytes, first_ordinal: int = 0) -> DeviceCSR:
        """One chunk (at most chunk_bytes) of text."""
        return self._wrap(self._p.parse(bytes(data), int(first_ordinal), 0, 0, 0), 0, 0)

    def parse_slot(self, slot: int, nbytes: int, first_ordinal: int = 0, carry_rows: int = 0,
                   carry_nnz: int = 0) -> DeviceCSR:
        """The first `nbytes` of pinned staging buffer `slot` (filled in place by a reader)."""
        return self._wrap(self._p.parse(int(slot), int(first_ordinal), int(nbytes), int(carry_rows), int(carry_nnz)),
                          carry_rows, carry_nnz)

    def fill_chunks(self, files: Sequence[str], loop: bool, take_slot, stopped=lambda: False):
        """Reads `files` in order into the pinned buffers and yields (slot, nbytes) per
        chunk: a chunk is cut at its last newline and the tail moves to the front of the
        next buffer; a file's end closes a chunk.  `take_slot()` hands out the next free
        buffer.  A line longer than chunk_bytes raises ValueError naming the file."""
        cap = self.chunk_bytes
        while not stopped():
            for f in files:
                path = gfile.local_path(f)
                fh = open(path, "rb", buffering=0) if path is not None else gfile.GFile(f, "rb")
                with fh:
                    tail = b""
                    eof = False
                    while not eof and not stopped():
                        slot = take_slot()
                        if slot is None:
                            return
                        buf = self._stage[slot]
                        n = len(tail)
                        buf[:n] = np.frombuffer(tail, np.uint8)
                        while n < cap:
                            if hasattr(fh, "readinto"):
                                k = fh.readinto(memoryview(buf)[n:cap])
                            else:
                                got = fh.read(cap - n)
                                k = len(got)
                                buf[n:n + k] = np.frombuffer(got, np.uint8)
                            if not k:
                                eof = True
                                break
                            n += k
                        tail = b""
                        if not eof:
                            cut = _after_last_newline(buf, n)
                            if cut == 0:
                                more = fh.read(1)
                                if more:
                                    raise ValueError(f"{f}: a line is longer than chunk_bytes = {cap}")
                                eof = True
                            else:
                                tail = buf[cut:n].tobytes()
                                n = cut
                        if n:
                            yield slot, n
            if not loop or not files:
                return

    def parse_files(self, files: Sequence[str]):
        """`DeviceCSR` chunks of the files in order; the ordinal runs over all of them."""
        out, ordinal, slot = [], 0, [1]

        def take():
            slot[0] ^= 1
            return slot[0]

        for s, n in self.fill_chunks(files, False, take):
            d = self.parse_slot(s, n, ordinal)
            ordinal += d.lines
            out.append(d)
        return out


class GpuBatchStream:
    """queue mode on the GPU parser: one reader thread fills the two pinned buffers
    while the consumer parses the other one; iterating yields device batches of
    exactly batch_size rows (rows left after a chunk's last whole batch are
    carried, on the device, into the next chunk's first batch); only the last
    batch of a non-looping stream may be short."""

    def __init__(self, parser: GpuLibsvmParser, files: Sequence[str], loop: bool = False):
        self.parser, self.files, self.loop = parser, list(files), loop
        self._free, self._full = queue.Queue(), queue.Queue()
        self._free.put(0)
        self._free.put(1)
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._read, daemon=True)
        self._thread.start()
        self._it = self._batches()
        self.rows_emitted = 0

    def _take(self):
        while not self._stop.is_set():
            try:
                return self._free.get(timeout=0.05)
            except queue.Empty:
                continue
        return None

    def _read(self):
        try:
            for item in self.parser.fill_chunks(self.files, self.loop, self._take, self._stop.is_set):
                self._full.put(item)
            self._full.put(None)
        except BaseException as e:  # noqa: BLE001 (handed to the consumer)
            self._full.put(e)

    def _batches(self):
        import torch

        bs = self.parser.batch_size
        carry, c, cnnz, ordinal = None, 0, 0, 0
        while True:
            item = self._full.get()
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            slot, n = item
            d = self.parser.parse_slot(slot, n, ordinal, c, cnnz)
            self._free.put(slot)                 # parse() returned: the buffer is consumed
            ordinal += d.lines
            for b in range(d.num_batches):
                y, off, ids, vals = d.batch(b)
                if b == 0 and c:
                    y = torch.cat([carry[0], y])
                    off = torch.cat([carry[1][:c], off])
                    ids, vals = torch.cat([carry[2], ids]), torch.cat([carry[3], vals])
                if y.shape[0] == bs:
                    carry, c, cnnz = None, 0, 0
                    self.rows_emitted += bs
                    yield y, off, ids, vals
                else:                            # the chunk's last, short batch: carried
                    carry, c, cnnz = (y, off, ids, vals), int(y.shape[0]), int(ids.shape[0])
        if c:
            self.rows_emitted += c
            yield carry

    def next(self):
        """The next batch, or None at the end of a non-looping stream."""
        return next(self._it, None)

    def stop(self):
        self._stop.set()
        while self._thread.is_alive():
            try:                                  # a reader blocked on a full hand-off
                self._full.get_nowait()
            except queue.Empty:
                pass
            self._thread.join(0.05)


def split_file_list(spec: str, num_workers: int = 1, task_index: int = 0) -> List[str]:
    """`files[task_index::num_workers]` of lr2.py:302-304.  `spec` is a comma
    list, or `@listfile` (one path per line, run.sh / lr2_debug.py:220-224),
    or a glob."""
    spec = spec.strip()
    if spec.startswith("@"):
        with gfile.GFile(spec[1:], "r") as f:
            files = [l.strip() for l in f if l.strip()]
    else:
        files = [f.strip() for f in spec.strip(",").split(",") if f.strip()]
        out = []
        for f in files:
            out.extend(sorted(gfile.Glob(f)) if any(c in f for c in "*?[") else [f])
        files = out
    return files[task_index::num_workers]


class DataProvider:
    """Per-worker sparse data facade with the reference's method names."""

    def __init__(self, num_workers: int, task_index: int, thread_num: int = 2, mode: str = "all",
                 train: str = "", test: str = "", batch_size: int = 500, train_sampling_rate: float = 1.0,
                 test_sampling_rate: float = 1.0, queue_capacity: int = 16, seed: int = 0, parser: str = "cpu",
                 device=None, chunk_bytes: int = 16 << 20):
        """`parser="gpu"`: the files are parsed on `device` (GpuLibsvmParser).  'all' mode
        brings the result back as CSRData, so shuffling and `take` stay as they are;
        'queue' mode's NextBatch yields device tuples (labels, offsets, ids, vals) of
        exactly batch_size rows, in file order, which train_step / evaluate /
        auc_update / evaluate_stream accept as they are."""
        if mode not in ("all", "queue"):
            raise ValueError("mode must be 'all' or 'queue'")
        if parser not in ("cpu", "gpu"):
            raise ValueError("parser must be 'cpu' or 'gpu'")
        self.parser, self.device, self.chunk_bytes = parser, device, int(chunk_bytes)
        self._gpu_parsers = {}
        self.mode, self.num_workers, self.task_index = mode, num_workers, task_index
        self.thread_num = max(1, int(thread_num))
        self.batch_size = int(batch_size)
        self.train_spec, self.test_spec = train, test
        self.train_rate, self.test_rate = train_sampling_rate, test_sampling_rate
        self.queue_capacity = queue_capacity
        self.rng = np.random.default_rng(seed + task_index)
        self.seed = seed
        self.train_file_list: List[str] = []
        self.test_file_list: List[str] = []
        self.train: Optional[CSRData] = None
        self.test: Optional[CSRData] = None
        self._order = None
        self._streams = {}

    # ------------------------------------------------------------ lifecycle
    def init(self, sess=None):
        self.train_file_list = split_file_list(self.train_spec, self.num_workers, self.task_index) \
            if self.train_spec else []
        self.test_file_list = split_file_list(self.test_spec, self.num_workers, self.task_index) \
            if self.test_spec else []
        return self

    def LoadData(self):  # noqa: N802 (reference name)
        t0 = time.time()
        if self.mode == "all":
            if self.parser == "gpu":
                for kind, files, rate, seed in (("train", self.train_file_list, self.train_rate, self.seed),
                                                ("test", self.test_file_list, self.test_rate, self.seed + 7919)):
                    gp = self._gpu_parsers[kind] = GpuLibsvmParser(self.device, self.chunk_bytes, self.batch_size,
                                                                   float(rate), int(seed))
                    setattr(self, kind, CSRData.concat([d.to_host() for d in gp.parse_files(files)]))
            else:
                self.train = load_files(self.train_file_list, self.thread_num, self.train_rate, self.seed)
                self.test = load_files(self.test_file_list, self.thread_num, self.test_rate, self.seed + 7919)
            self._order = np.arange(len(self.train))
            log.info(f"[worker:{self.task_index}] loaded {len(self.train)} train / {len(self.test)} test "
                     f"samples from {len(self.train_file_list)}+{len(self.test_file_list)} files "
                     f"in {time.time() - t0:.2f}s")
        else:
            C = _native.load()
            for kind, files, rate in (("train", self.train_file_list, self.train_rate),
                                      ("test", self.test_file_list, self.test_rate)):
                local = [gfile.local_path(f) or f for f in files]
                if files and self.parser == "gpu":
                    gp = GpuLibsvmParser(self.device, self.chunk_bytes, self.batch_size, float(rate), int(self.seed))
                    self._gpu_parsers[kind] = gp
                    self._streams[kind] = GpuBatchStream(gp, files, loop=True)
                elif files:
                    self._streams[kind] = C.LibsvmStream(local, self.batch_size, self.thread_num, float(rate),
                                                         True, int(self.queue_capacity), int(self.seed))
        return self

    def close(self):
        for s in self._streams.values():
            s.stop()
        self._streams.clear()

    def parser_stats(self) -> dict:
        """gpu_chunks / fallback_chunks / bad_lines summed over this provider's GPU parsers."""
        ps = self._gpu_parsers.values()
        return {"gpu_chunks": sum(p.gpu_chunks for p in ps), "fallback_chunks": sum(p.fallback_chunks for p in ps),
                "bad_lines": sum(p.bad_lines for p in ps)}

    # ------------------------------------------------------------ accessors
    def GetTrainSamples(self) -> CSRData:  # noqa: N802
        return self.train

    def GetTestSamples(self) -> CSRData:  # noqa: N802
        return self.test

    def Shuffle(self):  # noqa: N802
        if self._order is not None:
            self.rng.shuffle(self._order)

    def NextBatch(self, data_type: str = "train", max_batches: Optional[int] = None) -> Iterator[CSRBatch]:  # noqa: N802
        if self.mode == "all":
            data = self.train if data_type == "train" else self.test
            order = self._order if data_type == "train" else np.arange(len(data))
            n = len(data)
            for k, s in enumerate(range(0, n, self.batch_size)):
                if max_batches is not None and k >= max_batches:
                    return
                yield data.take(order[s:s + self.batch_size])
        else:
            st = self._streams.get(data_type)
            if st is None:
                return
            k = 0
            while max_batches is None or k < max_batches:
                b = st.next() if self.parser == "gpu" else st.next(30.0)
                if b is None:
                    return
                if self.parser == "gpu":
                    yield b
                    k += 1
                    continue
                y, rp, ids, vals = b
                yield CSRBatch(np.asarray(y, np.float32).reshape(-1, 1), rp, ids, vals)
                k += 1

    def GetTestSamplesSampled(self, sampling_rate: float = 1.0, sampling_max_num: int = 1000000) -> CSRBatch:  # noqa: N802
        if self.mode == "all":
            n = len(self.test)
            k = min(sampling_max_num, int(sampling_rate * n))
            rows = self.rng.choice(n, size=k, replace=False) if k else np.zeros(0, np.int64)
            return self.test.take(np.sort(rows))
        parts = []
        for b in self.NextBatch("test", max_batches=max(1, sampling_max_num // self.batch_size)):
            if isinstance(b, tuple):             # parser="gpu": device tensors
                b = CSRBatch(*(t.cpu().numpy() for t in b))
            parts.append(CSRData(b.labels, b.offsets, b.ids, b.vals))
        d = CSRData.concat(parts)
        return d.slice(0, len(d))


def write_synthetic(path_prefix: str, num_files: int, rows_per_file: int, num_features: int,
                    nnz_per_row: int = 20, seed: int = 0, zipf_a: float = 1.2) -> List[str]:
    """Synthetic libsvm shards with a planted linear model (power-law ids) --
    the stand-in for the reference's HDFS click logs (no dataset access)."""
    rng = np.random.default_rng(seed)
    w_true = rng.standard_normal(min(num_features, 1 << 22)).astype(np.float32)
    files = []
    os.makedirs(os.path.dirname(os.path.abspath(path_prefix)) or ".", exist_ok=True)
    for f in range(num_files):
        nnz = rng.integers(max(1, nnz_per_row // 2), nnz_per_row * 3 // 2 + 1, rows_per_file)
        ids = (rng.zipf(zipf_a, int(nnz.sum())) - 1) % num_features
        vals = np.round(rng.random(len(ids)) + 0.5, 3).astype(np.float32)
        offs = np.concatenate([[0], np.cumsum(nnz)])
        logit = np.add.reduceat(w_true[ids % len(w_true)] * vals, offs[:-1]) * 0.5
        y = (rng.random(rows_per_file) < 1 / (1 + np.exp(-logit))).astype(int)
        p = f"{path_prefix}-{f:05d}"
        with open(p, "w") as fh:
            for r in range(rows_per_file):
                s, e = offs[r], offs[r + 1]
                fh.write(f"{y[r]} " + " ".join(f"{i}:{v:g}" for i, v in zip(ids[s:e], vals[s:e])) + "\n")
        files.append(p)
    return files
