"""The GPU libsvm parser (csrc/kernels/libsvm_parse.hip) against the C++ parser.

The rule is bit-equality with `libsvm_parse_bytes`: regular text must come out
of the kernels (fallback_chunks == 0 is asserted, so a fallback cannot hide a
wrong kernel) with the same labels, offsets, ids and values; every construct
outside the kernels' grammar must send its chunk to the host parser
(fallback_chunks == 1) and so give the C++ parser's result, dropped lines and
bad_lines included.  Sizes sit on the tile edges (T = the tile bytes the
binding exports), batch sizes around the row count.
"""
import os

import numpy as np
import pytest
import torch

import libsvm_gpu_reference as R
from distributed_tensorflow_example_amd.data import libsvm

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CHUNK = 1 << 20


@pytest.fixture(scope="module")
def C(native):
    return native


@pytest.fixture(scope="module")
def T(C):
    return int(C.LIBSVM_GPU_TILE)


_parsers = {}


def parser(bs=500, rate=1.0, seed=0, chunk=CHUNK):
    key = (bs, rate, seed, chunk)
    if key not in _parsers:
        _parsers[key] = libsvm.GpuLibsvmParser(DEV, chunk, bs, rate, seed)
    return _parsers[key]


def cpu_parse(C, data):
    y, rp, ids, vals = C.libsvm_parse_bytes(bytes(data), 1.0, 0)
    return libsvm.CSRData(y, rp, ids, vals)


def same_csr(a, b):
    return (np.array_equal(R.bits32(a.labels), R.bits32(b.labels)) and np.array_equal(a.offsets, b.offsets)
            and np.array_equal(a.ids, b.ids) and np.array_equal(R.bits32(a.vals), R.bits32(b.vals)))


def check_regular(C, data, bs=500):
    """data through the kernels (no fallback) == the C++ parser, whole and batch by batch."""
    assert not R.Model().parse(data)["irregular"], "the fixture is not regular text"
    p = parser(bs)
    g0, f0 = p.gpu_chunks, p.fallback_chunks
    d = p.parse_bytes(data)
    assert p.fallback_chunks == f0 and p.gpu_chunks == g0 + 1 and not d.irregular and d.bad_lines == 0
    want = cpu_parse(C, data)
    assert d.lines == len(R.pieces(data))
    assert len(d) == len(want) and d.nnz == len(want.ids)
    assert same_csr(d.to_host(), want)
    assert d.num_batches == -(-len(want) // bs) and len(d.bases) == d.num_batches + 1
    for b, (y, off, ids, vals) in enumerate(d.batches()):
        ref = want.slice(b * bs, min(len(want), (b + 1) * bs))
        assert y.shape == (ref.size, 1) and off.dtype == torch.int64 and ids.dtype == torch.int64
        assert np.array_equal(R.bits32(y.cpu().numpy().reshape(-1)), R.bits32(ref.labels.reshape(-1)))
        assert np.array_equal(off.cpu().numpy(), ref.offsets)
        assert np.array_equal(ids.cpu().numpy(), ref.ids)
        assert np.array_equal(R.bits32(vals.cpu().numpy()), R.bits32(ref.vals))
    return d


def regular_text(n, seed=0):
    """Exactly n bytes of regular lines (the last one padded with blanks or cut short at a
    token boundary by blanks)."""
    rng = np.random.default_rng(seed)
    out = b""
    while len(out) < n:
        k = int(rng.integers(0, 6))
        line = f"{int(rng.integers(0, 2))} " + " ".join(
            f"{int(rng.integers(0, 10 ** int(rng.integers(1, 10))))}:{rng.integers(0, 2000) / 8:g}" for _ in range(k))
        out += line.rstrip().encode() + b"\n"
    if len(out) > n:                    # cut, then blank the partial last line from its last token boundary
        out = bytearray(out[:n])
        j = n
        while j > 0 and out[j - 1] not in b" \n":
            j -= 1
        out[j:n] = b" " * (n - j)
        # a line of blanks only is irregular: let it keep its label
        s = out.rfind(b"\n", 0, n) + 1
        if n - s >= 2 and not bytes(out[s:n]).strip():
            out[s:s + 1] = b"1"
        out = bytes(out)
    assert len(out) == n
    return out


HAND = (b"1 3:0.5 7:1.25\n"
        b"\t 0  \t 4:2\t\t5:3   \n"                 # tabs, runs of blanks, leading and trailing ws
        b"-1 1:1\r\n"                                 # CRLF
        b"\n"                                         # empty line
        b"7\n"                                        # 1-byte line: skipped
        b"\r\n"                                       # 1-byte line (CR)
        b"-1\n"                                       # label only
        b"+1 0:0 1:-0 2:+1.5 3:.5 4:5. 5:1E+3 6:1e-5\n"
        b"0 999999999999999999:123456789012345 8:1.23456789012345e22 9:1e-22 10:123456789012345e-22 11:-123456789.012345E+8\n"
        b"1 11:1e22 12:0.5e-21 13:00012.50 14:-.25e+1\n"
        b"0.5 3:1 \r\n"
        b"1 2:3")                                     # no final newline


def test_hand_built_file(C):
    d = check_regular(C, HAND)
    assert len(d) == 9
    check_regular(C, HAND, bs=1)
    check_regular(C, HAND + b"\n")


def test_write_synthetic_shards(C, tmp_path):
    files = libsvm.write_synthetic(str(tmp_path / "part"), 2, 400, 5000, nnz_per_row=20, seed=3)
    for f in files:
        with open(f, "rb") as fh:
            check_regular(C, fh.read(), bs=128)
    got = libsvm.load_files(files, parser="gpu", device=DEV)
    assert same_csr(got, libsvm.load_files(files, nthreads=1))


@pytest.mark.parametrize("which", ["0", "1", "T-1", "T", "T+1", "3T+5", "2T-1", "2T"])
def test_sizes_at_the_tile_edges(C, T, which):
    n = {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5, "2T-1": 2 * T - 1, "2T": 2 * T}[which]
    check_regular(C, regular_text(n, seed=n), bs=16)
    if n == 1:
        check_regular(C, b"\n")
        check_regular(C, b"5")


@pytest.mark.parametrize("what", ["token", "colon", "newline"])
@pytest.mark.parametrize("at", ["last", "first"])
def test_a_byte_on_the_tile_boundary(C, T, what, at):
    p = T - 1 if at == "last" else T
    if what == "token":       # the entry's first byte at p
        text = b"1" + b" " * (p - 1) + b"3:0.5 4:1\n"
        assert text[p:p + 1] == b"3"
    elif what == "colon":
        text = b"1" + b" " * (p - 2) + b"3:0.5 4:1\n"
        assert text[p:p + 1] == b":"
    else:
        text = b"1 3:0.5" + b" " * (p - 7) + b"\n"
        assert text[p:p + 1] == b"\n"
    check_regular(C, text + b"0 4:2 5:1\n-1\n1 6:.5\n", bs=2)


def test_a_line_longer_than_two_tiles(C, T):
    entries = " ".join(f"{100000 + k}:{k}.25" for k in range(2 * T // 12 + 300))
    text = f"1 2:1\n0 {entries}\n1 3:1\n".encode()
    assert text.count(b":") >= 300 and len(text) > 2 * T + 12
    d = check_regular(C, text, bs=2)
    assert len(d) == 3


def test_no_newline_and_no_entries(C):
    check_regular(C, b"1 3:0.5 4:1")
    check_regular(C, b"1\n0\n-1\n")
    check_regular(C, b"\n\n\n\n")
    check_regular(C, b" 1")


@pytest.mark.parametrize("bs", ["1", "7", "R-1", "R", "R+1"])
def test_batch_sizes_around_the_row_count(C, bs):
    text = regular_text(1500, seed=77)
    rows = len(cpu_parse(C, text))
    assert rows > 20
    check_regular(C, text, bs={"1": 1, "7": 7, "R-1": rows - 1, "R": rows, "R+1": rows + 1}[bs])


def test_many_lines_cross_the_line_tile(C):
    text = b"".join(b"%d %d:%d.5\n" % (k % 2, k, k % 9) if k % 5 else b"%d\n" % (k % 2) for k in range(3000))
    check_regular(C, text, bs=1000)


# ------------------------------------------------------------------ irregular
CLEAN = b"1 3:0.5 7:1.25\n0 4:2\n"
IRREGULAR = {
    "inf": b"1 3:inf\n", "nan": b"nan 3:1\n", "hex float": b"1 3:0x1p3\n", "blank after colon": b"1 3: 0.5\n",
    "two colons": b"1 3:4:5\n", "no value": b"1 3:\n", "no index": b"1 :5\n", "open exponent": b"1 3:1e\n",
    "signed index": b"1 +3:1\n", "negative index": b"1 -3:1\n", "19-digit index": b"1 1234567890123456789:1\n",
    "blank line": b"   \n", "two CRs": b"\r\r\n", "control byte": b"1 3:1\x01\n", "high byte": b"1 3:1\x80\n",
    "NUL": b"1 3:1\x00 4:1\n", "1e40": b"1 3:1e40\n", "1e-40": b"1 3:1e-40\n", "float tie": b"1 3:16777217\n",
    "16 digits": b"1 3:1234567890123456\n", "1e23": b"1 3:1e23\n", "label with colon": b"3:1 4:1\n",
    "bare number entry": b"1 2\n", "trailing letters": b"1 3:0.5abc\n", "vertical tab": b"1\v3:1\n",
    "label 1e": b"1e 3:1\n",
}


@pytest.mark.parametrize("name", sorted(IRREGULAR))
def test_irregular_chunk_falls_back_to_the_cpp_parser(C, name):
    data = CLEAN + IRREGULAR[name] + CLEAN * 2
    p = libsvm.GpuLibsvmParser(DEV, 4096, 3)
    d = p.parse_bytes(data)
    assert p.fallback_chunks == 1 and p.gpu_chunks == 0 and d.irregular
    assert R.Model().parse(data)["irregular"]
    want = cpu_parse(C, data)
    assert same_csr(d.to_host(), want)
    bad = C.libsvm_parse_bytes_hashed(data, 1.0, 0, 0)[5]
    assert p.bad_lines == bad == d.bad_lines and len(want) == 6 + (1 - bad)
    for b, (y, off, ids, vals) in enumerate(d.batches()):
        ref = want.slice(b * 3, min(len(want), (b + 1) * 3))
        assert np.array_equal(off.cpu().numpy(), ref.offsets) and np.array_equal(ids.cpu().numpy(), ref.ids)
    # the parser goes on with the kernels for the next, clean chunk
    p.parse_bytes(CLEAN)
    assert p.gpu_chunks == 1 and p.fallback_chunks == 1


# ------------------------------------------------------------------- sampling
def test_sampling_keeps_exactly_the_models_lines(C):
    rng = np.random.default_rng(8)
    lines = []
    for k in range(10_000):
        if k % 211 == 0:
            lines.append(b"")
        elif k % 223 == 0:
            lines.append(b"3")
        else:
            lines.append(b"%d " % (k % 2) + b" ".join(b"%d:%d.5" % (int(i), k) for i in rng.integers(0, 999, k % 4)))
    data = b"\n".join(lines) + b"\n"
    seed, first, rate = 99, 1234, 0.3
    p = parser(64, rate, seed)
    d = p._wrap(p._p.parse(data, first, 0, 0, 0), 0, 0)
    assert p.fallback_chunks == 0
    m = R.Model().parse(data, rate, seed, first)
    assert not m["irregular"] and 2700 < len(m["kept"]) < 3300
    want = cpu_parse(C, b"\n".join(lines[o - first] for o in m["kept"]) + b"\n")
    assert len(d) == len(m["kept"]) and same_csr(d.to_host(), want)
    h = C.libsvm_parse_bytes_hashed(data, rate, seed, first)
    assert same_csr(libsvm.CSRData(*h[:4]), want)                       # the host form keeps the same sample
    d2 = p._wrap(p._p.parse(data, first, 0, 0, 0), 0, 0)
    assert torch.equal(d.labels, d2.labels) and torch.equal(d.offsets, d2.offsets)
    assert torch.equal(d.ids, d2.ids) and torch.equal(d.vals.view(torch.int32), d2.vals.view(torch.int32))
    # an irregular chunk at rate < 1: the hashed host parser, the same sample
    data2 = data + b"1 3:inf\n"
    d3 = p._wrap(p._p.parse(data2, first, 0, 0, 0), 0, 0)
    h3 = C.libsvm_parse_bytes_hashed(data2, rate, seed, first)
    assert d3.irregular and same_csr(d3.to_host(), libsvm.CSRData(*h3[:4]))


# ------------------------------------------------- the launcher on caller's tensors
GUARD = 64   # elements around every buffer


class Buffers:
    """The launcher's tensors for n bytes, each inside guard bands, pre-filled."""

    def __init__(self, C, n, bs, carry=0, ws_fill=0xFF, slack=0):
        plan = C.libsvm_gpu_plan(n, bs, carry)
        self.plan = plan
        sizes = {"text": (max(n, 1) + 15) // 16 * 16, "workspace": plan["workspace_bytes"] + slack,
                 "labels": plan["rows"], "ids": plan["nnz"], "vals": plan["nnz"],
                 "offsets": plan["batches"] * (bs + 1), "meta": plan["meta"]}
        dt = {"text": torch.uint8, "workspace": torch.uint8, "labels": torch.float32, "ids": torch.int64,
              "vals": torch.float32, "offsets": torch.int64, "meta": torch.int64}
        self.fill = {"text": 0x7F, "workspace": ws_fill, "labels": float("nan"), "ids": -7, "vals": float("nan"),
                     "offsets": -7, "meta": -7}
        self.full, self.view = {}, {}
        for k, sz in sizes.items():
            self.full[k] = torch.full((sz + 2 * GUARD,), self.fill[k], dtype=dt[k], device=DEV)
            self.view[k] = self.full[k][GUARD:GUARD + sz]

    def set_text(self, data):
        if len(data):
            self.view["text"][:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))

    def args(self):
        v = self.view
        return v["workspace"], v["labels"], v["ids"], v["vals"], v["offsets"], v["meta"]

    def guards_intact(self):
        for k, t in self.full.items():
            for band in (t[:GUARD], t[-GUARD:]):
                if k in ("labels", "vals"):
                    if not bool(torch.isnan(band).all()):
                        return False
                elif not bool((band == self.fill[k]).all()):
                    return False
        return True

    def result(self, bs):
        meta = self.view["meta"].cpu().numpy()
        rows, nnz, irregular, lines, nb = int(meta[0]), int(meta[1]), int(meta[2]), int(meta[3]), int(meta[6])
        assert not irregular
        d = libsvm.DeviceCSR(self.view["labels"][:rows], self.view["offsets"][:nb * (bs + 1)].view(nb, bs + 1),
                             self.view["ids"][:nnz], self.view["vals"][:nnz], meta[8:8 + nb + 1], bs, lines=lines)
        return d.to_host()


def test_prefilled_buffers_and_guard_bands(C, T):
    data = regular_text(2 * T + 100, seed=5)[:-1] + b"\n1 3:0.5"       # (the text ends in a blank or a newline)
    n, bs = len(data), 7
    assert not R.Model().parse(data)["irregular"]
    want = cpu_parse(C, data)
    for ws_fill in (0xFF, 0x00, 0x5A):
        B = Buffers(C, n, bs, ws_fill=ws_fill)
        B.set_text(data)
        C.libsvm_gpu_parse_into(B.view["text"], n, 0, 0, 1.0, bs, 0, 0, *B.args())
        torch.cuda.synchronize()
        assert B.guards_intact()
        assert same_csr(B.result(bs), want)
    # a hostile chunk (every byte a ':' / a newline): flagged, and nothing written out of bounds
    # and the densest regular ones: a line per 3 bytes, an entry per 4
    for junk in (b":" * n, b"\n" * n, b"1\n" * (n // 2), b"1 :" * (n // 3), b"-1\n" * (n // 3), b"-1\n" * (n // 3) + b"-1",
                 b"1" + b" 1:1" * (n // 4)):
        B = Buffers(C, len(junk), bs)
        B.set_text(junk)
        C.libsvm_gpu_parse_into(B.view["text"], len(junk), 0, 0, 1.0, bs, 0, 0, *B.args())
        torch.cuda.synchronize()
        assert B.guards_intact()
        meta = B.view["meta"].cpu().numpy()
        if R.Model().parse(junk)["irregular"]:
            assert junk[:1] == b":" or junk[:3] == b"1 :"
            assert meta[2] == 1
        else:
            assert meta[2] == 0 and same_csr(B.result(bs), cpu_parse(C, junk))


def test_refusals_launch_nothing(C):
    data = CLEAN * 4
    n, bs = len(data), 4
    B = Buffers(C, n, bs)
    B.set_text(data)
    v = B.view
    bad_calls = [
        dict(n=1 << 31), dict(rate=0.0), dict(rate=1.5), dict(rate=float("nan")), dict(bs=0), dict(n=-1),
        dict(carry=bs), dict(labels=v["labels"].cpu()), dict(meta=v["meta"][:4]), dict(workspace=v["workspace"][:64]),
        dict(ids=v["ids"].to(torch.int32)),
    ]
    for kw in bad_calls:
        a = dict(n=n, rate=1.0, bs=bs, carry=0, workspace=v["workspace"], labels=v["labels"], ids=v["ids"],
                 vals=v["vals"], offsets=v["offsets"], meta=v["meta"])
        a.update(kw)
        with pytest.raises(Exception):
            C.libsvm_gpu_parse_into(v["text"], a["n"], 0, 0, a["rate"], a["bs"], a["carry"], 0, a["workspace"],
                                    a["labels"], a["ids"], a["vals"], a["offsets"], a["meta"])
    torch.cuda.synchronize()
    assert bool((B.full["meta"] == -7).all()) and bool(torch.isnan(B.full["labels"]).all())   # nothing ran
    assert bool((B.full["workspace"] == 0xFF).all())
    if torch.cuda.device_count() > 1:
        with pytest.raises(Exception):
            C.libsvm_gpu_parse_into(v["text"], n, 0, 0, 1.0, bs, 0, 0, v["workspace"], v["labels"].to("cuda:1"),
                                    v["ids"], v["vals"], v["offsets"], v["meta"])
    for ctor in (dict(chunk=1 << 31), dict(rate=0.0), dict(rate=1.01), dict(bs=0), dict(dev=torch.cuda.device_count())):
        with pytest.raises(Exception):
            C.LibsvmGpuParser(ctor.get("dev", 0), ctor.get("chunk", 4096), ctor.get("bs", 4), ctor.get("rate", 1.0), 0)
    p = libsvm.GpuLibsvmParser(DEV, 64, 4)
    with pytest.raises(Exception):
        p.parse_bytes(b"1 3:1\n" * 20)             # larger than chunk_bytes
    assert p.gpu_chunks == 0 and p.fallback_chunks == 0


def test_graph_replay_gives_the_same_bits(C, T):
    a = regular_text(T + 300, seed=21)
    b = regular_text(T + 300, seed=22)
    n, bs = len(a), 5
    B = Buffers(C, n, bs)
    B.set_text(a)
    call = lambda: C.libsvm_gpu_parse_into(B.view["text"], n, 0, 0, 1.0, bs, 0, 0, *B.args())  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = B.result(bs)
    assert same_csr(eager, cpu_parse(C, a))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for text in (b, a, b):
        B.set_text(text)
        for k in ("labels", "vals"):
            B.view[k].fill_(float("nan"))
        B.view["meta"].fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert same_csr(B.result(bs), cpu_parse(C, text))
        assert B.guards_intact()


# --------------------------------------------------------------- DataProvider
def _write_files(tmp_path):
    # (regular_text ends in a blank or a newline: "b" closes that line before its last, unterminated one)
    specs = [(regular_text(9000, seed=31), "a"), (regular_text(5000, seed=32)[:-1] + b"\n1 3:0.5 9:2", "b"),
             (regular_text(4096 * 2, seed=33), "c")]
    files = []
    for data, name in specs:
        assert not R.Model().parse(data)["irregular"], "the fixture is not regular text"
        f = str(tmp_path / f"part-{name}")
        with open(f, "wb") as fh:
            fh.write(data)
        files.append(f)
    return files, [s[0] for s in specs]


def test_data_provider_queue_mode_on_the_gpu_parser(C, tmp_path):
    files, datas = _write_files(tmp_path)
    bs = 37
    one = libsvm.CSRData.concat([cpu_parse(C, d) for d in datas])
    want = libsvm.CSRData.concat([one, one, one])            # loop=True wraps around the files
    nbatches = (2 * len(one)) // bs + 2                      # past one wrap
    dp = libsvm.DataProvider(1, 0, mode="queue", train=",".join(files), batch_size=bs, parser="gpu", device=DEV,
                             chunk_bytes=4096).init().LoadData()
    try:
        k = 0
        for y, off, ids, vals in dp.NextBatch("train", max_batches=nbatches):
            ref = want.slice(k * bs, (k + 1) * bs)
            assert y.is_cuda and y.shape == (bs, 1) and off.shape == (bs + 1,)
            assert np.array_equal(R.bits32(y.cpu().numpy().reshape(-1)), R.bits32(ref.labels.reshape(-1))), k
            assert np.array_equal(off.cpu().numpy(), ref.offsets), k
            assert np.array_equal(ids.cpu().numpy(), ref.ids), k
            assert np.array_equal(R.bits32(vals.cpu().numpy()), R.bits32(ref.vals)), k
            k += 1
        assert k == nbatches
        st = dp.parser_stats()
        assert st["fallback_chunks"] == 0 and st["gpu_chunks"] >= 7 and st["bad_lines"] == 0
    finally:
        dp.close()
    # a non-looping stream ends with the one short batch
    gp = libsvm.GpuLibsvmParser(DEV, 4096, bs)
    st = libsvm.GpuBatchStream(gp, files, loop=False)
    sizes = []
    while True:
        b = st.next()
        if b is None:
            break
        sizes.append(int(b[0].shape[0]))
    st.stop()
    assert sum(sizes) == len(one) and all(s == bs for s in sizes[:-1]) and 0 < sizes[-1] <= bs
    # 'all' mode: parsed on the GPU, served from the host as before
    dpa = libsvm.DataProvider(1, 0, thread_num=1, mode="all", train=",".join(files), test=files[0], batch_size=bs,
                              parser="gpu", device=DEV, chunk_bytes=4096).init().LoadData()
    assert same_csr(dpa.GetTrainSamples(), one) and same_csr(dpa.GetTestSamples(), cpu_parse(C, datas[0]))
    assert dpa.parser_stats()["fallback_chunks"] == 0


def test_a_line_longer_than_the_chunk_names_the_file(C, tmp_path):
    f = str(tmp_path / "long-line")
    with open(f, "wb") as fh:
        fh.write(b"1 3:1\n0 " + b" ".join(b"%d:1" % k for k in range(1500)) + b"\n1 4:1\n")
    dp = libsvm.DataProvider(1, 0, mode="queue", train=f, batch_size=2, parser="gpu", device=DEV,
                             chunk_bytes=4096).init().LoadData()
    try:
        with pytest.raises(ValueError, match="long-line"):
            for _ in dp.NextBatch("train", max_batches=10):
                pass
    finally:
        dp.close()


# ------------------------------------------------------------- sparse LR end to end
@pytest.mark.parametrize("optimizer", ["sgd", "ftrl"])
def test_sparse_lr_trains_to_the_same_bits_on_gpu_parsed_batches(C, tmp_path, optimizer):
    """W and b after 20 steps on GPU-parsed device batches == 20 steps on CPU-parsed ones, bit for bit.

    The fused step (csrc/kernels/sparse_lr.hip) sums the updates of an id that occurs
    several times in a batch with float atomics, in an order that is not fixed: on
    such batches two runs of the same trainer on the same bits differ in the last
    bits (measured on an MI355X with write_synthetic's power-law ids, three trainers
    fed the same CPU-parsed batches for 20 steps: SGD 3 and 6 weights apart by up to
    7 ulp, FTRL 254 and 337 weights).
    So the shards here hold every id at most once per batch: each weight then
    receives one addend per step, the step is a function of its input bits alone,
    and a differing bit can only come from the parser."""
    from distributed_tensorflow_example_amd.models import sparse_lr
    from distributed_tensorflow_example_amd.parallel.world import World

    F, bs, steps, per_row, rows_per_file = 5000, 50, 20, 12, 600
    rng = np.random.default_rng(4)
    files = []
    for f in range(2):
        path = str(tmp_path / f"part-{f}")
        with open(path, "w") as fh:
            for _ in range(rows_per_file // bs):
                ids = rng.permutation(F)[:bs * per_row].reshape(bs, per_row)      # distinct within the batch
                for row in ids:
                    fh.write(f"{int(rng.integers(0, 2))} " +
                             " ".join(f"{int(i)}:{rng.integers(500, 1500) / 1000:g}" for i in row) + "\n")
        files.append(path)
    host = libsvm.load_files(files, nthreads=1)
    assert len(host) == 2 * rows_per_file
    for k in range(len(host) // bs):
        b = host.slice(k * bs, (k + 1) * bs)
        assert len(np.unique(b.ids)) == len(b.ids)

    def trainer():
        return sparse_lr.SparseLRTrainer(F, 0.1, World(device=DEV), seed=2, optimizer=optimizer)

    def gpu_batches():
        gp = libsvm.GpuLibsvmParser(DEV, 8192, bs)
        st = libsvm.GpuBatchStream(gp, files, loop=False)
        try:
            while True:
                b = st.next()
                if b is None:
                    return
                yield b
        finally:
            st.stop()
            assert gp.fallback_chunks == 0 and gp.gpu_chunks >= 2

    ta, tb = trainer(), trainer()
    gb = gpu_batches()
    for k in range(steps):
        ta.train_step(host.slice(k * bs, (k + 1) * bs).to(DEV))
        tb.train_step(next(gb))
    torch.cuda.synchronize()
    assert torch.equal(ta.W.local.view(torch.int32), tb.W.local.view(torch.int32))
    assert torch.equal(ta.b.data.view(torch.int32), tb.b.data.view(torch.int32))
    rest = list(gb)
    assert len(rest) == len(host) // bs - steps
    ra = ta.evaluate_stream([host.slice(k * bs, (k + 1) * bs).to(DEV) for k in range(steps, len(host) // bs)])
    rb = tb.evaluate_stream(rest)
    assert ra == rb and ra["rows"] == len(host) - steps * bs
