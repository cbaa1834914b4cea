"""What a store HOLDS, against a host-only model (oracle.radad_oracle.stored_rows / stored_rows_err).

The search tests take their oracle's inputs from the device ("the rows as stored" = reconstruct_batch, the cosine queries =
radad_rownorm): if ingest, gather and scan read the same wrong bytes they agree with themselves.  Here rows are made on the
host (oracle.synth), so host and device start from the same fp32 bits, and everything the device holds or writes -- after
add / add_device, after capacity growth and reserve, in a snapshot file, after load / load(range), inside an IVF store, and
the query a search really uses -- is compared with what the host model says, bit for bit where the operation is exact and
within a bound derived from the kernel's arithmetic where it rounds (cosine).  No store that holds +-inf is searched."""
import os
import struct

import numpy as np
import pytest

from oracle import radad_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu

BASE = 10 ** 10                     # id_base of the ingest tests: ids beyond 2^32
DIMS = [4, 8, 12, 28, 48, 64, 100, 252, 256, 260, 1024, 5376, 16380]  # nv = dim / 4 below, at and above 64 lanes; 1 to 64 trips of the lane
                                                                       # loop; 16380: the widest rows a search at k = 1024 takes
COUNTS = [1, 3, 4, 5, 1025]         # four rows per workgroup: part of one, exactly one, one and a bit, many and a bit
HEADER = struct.Struct("<8sIiiiq")  # "RADADKNN" | u32 version | i32 dim | i32 metric | i32 store dtype | i64 ntotal


def _lib():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib as L
    return L


def _mk(gpu, metric, dim, f16=False, id_base=0, **options):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex
    L = _lib()
    m = {"L2": L.METRIC_L2, "IP": L.METRIC_IP, "COSINE": L.METRIC_COSINE}[metric]
    return HipFlatIndex(dim, m, gpu.index or 0, id_base, store_f16=f16, **options)


def _assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits, first at {at}: "
                             f"device {got[at]!r} ({got.view(np.uint32)[at]:#010x}) model {want[at]!r} ({want.view(np.uint32)[at]:#010x})")


def _ratio(got, exact, bound):
    """worst |got - exact| / bound; an element with bound 0 must be met exactly (inf otherwise)"""
    err = np.abs(np.asarray(got, np.float64) - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def _held(idx, n, gpu, base=None):
    import torch
    base = idx.id_base if base is None else base
    return idx.reconstruct_batch(torch.arange(base, base + n, device=gpu)).cpu().numpy()


def _rownorm(gpu, x, out=None):
    import torch
    L = _lib()
    out = torch.empty_like(x) if out is None else out
    L.check(L.load().radad_rownorm(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], gpu.index or 0, L.stream_ptr(gpu)))
    return out


def _f16_model(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def _key_rtol(dim):
    """float64 sum of `dim` non-negative terms (q - y)^2, on the device and in the oracle, in any order: each within
    (dim + 2) 2^-53 of the exact value, relatively"""
    return 2 * (dim + 3) * 2.0 ** -53


# ---- a. ingest --------------------------------------------------------------------------------------------------------------

FP16_CASES = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65520.0, -65520.0, 65504.0, 65519.996, 1023 * 2.0 ** -24,
                       1023 * 2.0 ** -24 + 2.0 ** -25, 2.0 ** -25, 3 * 2.0 ** -25, -(1 + 2.0 ** -11), 2.0 ** -24], np.float32)


def _ingest_rows(dim, cosine):
    """1025 synthetic rows; rows 7..12 and the last are the hard ones (the first five stay ordinary: the small row counts)"""
    rows = synth.rows(0, 1025, dim, 9100 + dim)
    sign = np.where(np.arange(dim) % 3 == 1, -1.0, 1.0).astype(np.float32)
    rows[7] = np.resize(FP16_CASES, dim)                   # fp16 ties (to even, not away, not truncated), overflow, subnormals
    rows[8] = 0                                            # a zero row
    rows[9] = np.float32(2.0 ** -60) * sign                # squares are still normal fp32 numbers; under cosine the 1e-12 dominates
    rows[10] *= np.float32(2.0 ** 40)
    rows[11] *= np.float32(2.0 ** -40)
    if cosine:
        rows[12] = np.float32(2.0 ** 70) * sign * (1 + np.arange(dim) % 3).astype(np.float32)     # squares overflow fp32: norm inf
    rows[1024] = np.resize(FP16_CASES[::-1], dim)          # ... and in the workgroup that holds a single row
    return rows


@pytest.mark.parametrize("dim", DIMS)
def test_ingest_holds_what_the_model_says(gpu, dim):
    """add (host) and add_device, L2 / IP / cosine x fp32 / fp16 stores, row counts 1, 3, 4, 5, 1025, id_base 10^10.
    L2 / IP: reconstruct_batch and reconstruct(i) are bit-equal to stored_rows().  Cosine fp32: every element within
    stored_rows_err()'s bound of the float64 value (the message carries the worst error / bound); equal in bits to radad_rownorm
    of the same rows at every row count, and radad_rownorm in place == out of place.  Cosine fp16: np.float16 of the fp32
    store's own value.  Ids -1, below id_base and >= id_base + ntotal reconstruct to zeros."""
    import torch
    worst = 0.0
    for metric in ("L2", "IP", "COSINE"):
        cosine = metric == "COSINE"
        rows = _ingest_rows(dim, cosine)
        rows_t = torch.from_numpy(rows).to(gpu)
        if cosine:
            exact, bound = O.stored_rows_err(rows)
            assert np.all(exact[8] == 0) and np.all(exact[12] == 0) and np.all(bound[9] > 0)
            inplace = rows_t.clone()
            _rownorm(gpu, inplace, out=inplace)
            _assert_bits(inplace.cpu().numpy(), _rownorm(gpu, rows_t).cpu().numpy(), f"dim {dim}: radad_rownorm in place vs out of place")
        for n in COUNTS:
            held32 = None
            for f16 in (False, True):
                what = f"{metric} dim {dim} n {n} {'fp16' if f16 else 'fp32'} store"
                a = _mk(gpu, metric, dim, f16, id_base=BASE)
                a.add(rows[:n])
                b = _mk(gpu, metric, dim, f16, id_base=BASE)
                b.add_device(rows_t[:n])
                assert a.ntotal == n and b.ntotal == n
                ha, hb = _held(a, n, gpu), _held(b, n, gpu)
                _assert_bits(ha, hb, f"{what}: add vs add_device")
                if not cosine:
                    _assert_bits(ha, O.stored_rows(rows[:n], metric, f16).astype(np.float32), f"{what}: reconstruct_batch vs stored_rows")
                elif not f16:
                    r = _ratio(ha, exact[:n], bound[:n])
                    worst = max(worst, r)
                    assert r <= 1.0, (f"{what}: worst |stored - float64 model| / bound = {r:.3f} (bound (d/2 + 4) u |x|, "
                                      f"d = {O.cosine_sum_depth(dim)})")
                    _assert_bits(ha, _rownorm(gpu, rows_t[:n]).cpu().numpy(), f"{what}: cosine store vs radad_rownorm of the same rows")
                    held32 = ha
                else:
                    _assert_bits(ha, _f16_model(held32), f"{what}: fp16 cosine store vs np.float16 of the fp32 store's value")
                for i in sorted({0, n // 2, n - 1, min(7, n - 1), min(12, n - 1)}):
                    _assert_bits(a.reconstruct(BASE + i), ha[i], f"{what}: reconstruct({i})")
                ids = torch.tensor([-1, BASE - 1, BASE + n, BASE + n + 5, 0, n - 1, BASE], device=gpu)
                rec = a.reconstruct_batch(ids).cpu().numpy()
                assert not rec[:6].any(), f"{what}: ids outside [id_base, id_base + ntotal) must reconstruct to zeros"
                _assert_bits(rec[6], ha[0], f"{what}: id_base itself")
                for i in (-1, BASE - 1, BASE + n, 0):
                    assert not a.reconstruct(i).any(), f"{what}: reconstruct({i}) must be zeros"
    print(f"cosine ingest, dim {dim}: worst |stored - float64 model| / bound = {worst:.3f}")


# ---- b. the query a search uses ---------------------------------------------------------------------------------------------

def _probe_cols(dim, ncols):
    if ncols is None:
        ncols = min(dim, 1024)
    cols = np.unique(np.round(np.linspace(0, dim - 1, ncols)).astype(np.int64))
    assert len(cols) == ncols and cols[0] == 0 and cols[-1] == dim - 1
    return cols


def _probe_store(gpu, metric, dim, cols, **options):
    """rows e_c for the chosen columns: the float64 key of hit `id` is the prepared query's component cols[id] -- one product with
    1.0, the others with 0 -- and under cosine e_c / (1 + 1e-12f) is e_c in fp32"""
    store = np.zeros((len(cols), dim), np.float32)
    store[np.arange(len(cols)), cols] = 1.0
    idx = _mk(gpu, metric, dim, **options)
    idx.add(store)
    _assert_bits(_held(idx, len(cols), gpu), store, f"{metric} dim {dim}: unit rows as stored")
    return idx


def _probe_expect(prep, cols):
    """(ids, keys) a search with k = all rows must return for prepared queries `prep`: components in descending order, the lower id
    first among equal ones"""
    comp = np.asarray(prep)[:, cols].astype(np.float64)
    ids = np.broadcast_to(np.arange(len(cols), dtype=np.int64), comp.shape)
    order = np.lexsort((ids, -comp), axis=1)
    return order, np.take_along_axis(comp, order, 1)


# the scan each probe takes, from the host code (knn_plan_scan): k = all rows <= 1024 is beyond the f16 scans; a store of <= 6144 fp32
# rows whose dim is a multiple of 16 takes k_knn_dense whatever the batch; otherwise <= 16 queries with k + margin <= 32 and
# dim % 32 == 0 stream (f32_smallq), everything else takes the fp32 tile kernels.  The query preparation is k_hi_rows_wide (a
# workgroup per query) for <= 16 queries and k_hi_rows (a wave per query) above, whatever the scan.
PROBES = [(64, None, {}, "f32_dense", "f32_dense"),
          (100, None, {}, "f32_tile", "f32_tile"),
          (256, None, {}, "f32_dense", "f32_dense"),
          (260, None, {}, "f32_tile", "f32_tile"),
          (1024, None, {}, "f32_dense", "f32_dense"),
          (5376, 1024, {}, "f32_dense", "f32_dense"),
          (64, 8, {"dense": 0}, "f32_smallq", "f32_tile")]


@pytest.mark.parametrize("metric", ["IP", "COSINE"])
@pytest.mark.parametrize("dim,ncols,options,kind_small,kind_large", PROBES)
def test_the_query_a_search_uses(gpu, metric, dim, ncols, options, kind_small, kind_large):
    """IP: the float64 key of every hit is the input component, exactly.  Cosine: it is the float64 value of radad_rownorm(q), bit
    for bit (the contract k_hi_rows states: the three normalisation kernels give the same bits), and within stored_rows_err of
    the float64 model.  Batches of 1, 16, 17 and 300 queries: both forms of the query preparation."""
    import torch
    cols = _probe_cols(dim, ncols)
    n = len(cols)
    idx = _probe_store(gpu, metric, dim, cols, **options)
    q = synth.rows(0, 300, dim, 9300 + dim)
    q[2, cols[: min(4, n)]] = np.float32(0.5)                   # equal components: the lower id first
    q[3] *= np.float32(2.0 ** 20)
    q[5] *= np.float32(2.0 ** -20)
    q[6, cols[0]] = 0.0
    if metric == "COSINE":
        exact, bound = O.stored_rows_err(q)
    worst = 0.0
    for nq in (1, 16, 17, 300):
        qt = torch.from_numpy(q[:nq]).to(gpu)
        D, I, K = idx.search_device(qt, n, return_f64=True)
        kind = idx.last_launch()["scan_kind"]
        assert kind == (kind_small if nq <= 16 else kind_large), f"dim {dim} nq {nq}: scan {kind}"
        prep = q[:nq] if metric == "IP" else _rownorm(gpu, qt).cpu().numpy()
        oi, ok = _probe_expect(prep, cols)
        I, K, D = I.cpu().numpy(), K.cpu().numpy(), D.cpu().numpy()
        what = f"{metric} dim {dim} rows {n} nq {nq} ({kind})"
        np.testing.assert_array_equal(I, oi, err_msg=f"{what}: ids")
        bad = K != ok
        assert not bad.any(), (f"{what}: {int(bad.sum())} float64 keys differ from the prepared query's components, first at "
                               f"{tuple(np.argwhere(bad)[0])}: {K[bad][0]!r} vs {ok[bad][0]!r}")
        np.testing.assert_array_equal(D, ok.astype(np.float32), err_msg=f"{what}: distances")
        if metric == "COSINE":
            col_of = cols[I]
            r = _ratio(K, np.take_along_axis(exact[:nq], col_of, 1), np.take_along_axis(bound[:nq], col_of, 1))
            worst = max(worst, r)
            assert r <= 1.0, f"{what}: worst |key - float64 model| / bound = {r:.3f} (d = {O.cosine_sum_depth(dim)})"
    if metric == "COSINE":
        print(f"cosine query preparation, dim {dim} rows {n}: worst |key - float64 model| / bound = {worst:.3f}")


def _bf16_patterns():
    """every bf16 pattern with exponent 2^-30 .. 2^30, both signs, all 128 mantissas, and +-0: uint16 [62, 256] (zero padded)"""
    pats = [(s << 15) | (e << 7) | m for s in (0, 1) for e in range(127 - 30, 127 + 31) for m in range(128)] + [0x0000, 0x8000]
    assert len(pats) == 2 * 61 * 128 + 2
    arr = np.zeros(62 * 256, np.uint16)
    arr[:len(pats)] = pats
    return arr.reshape(62, 256)


def test_bf16_queries_are_decoded_exactly(gpu):
    import torch
    bits = _bf16_patterns()
    dec = (bits.astype(np.uint32) << 16).view(np.float32)               # bf16 is the upper half of an fp32
    assert np.isfinite(dec).all() and np.abs(dec[dec != 0]).min() == 2.0 ** -30 and np.abs(dec).max() == (2 - 2.0 ** -7) * 2.0 ** 30
    qb = torch.from_numpy(bits.view(np.int16)).to(gpu).view(torch.bfloat16)
    dim = 256
    cols = _probe_cols(dim, None)
    idx = _probe_store(gpu, "IP", dim, cols)
    for nq in (16, 62):
        D, I, K = idx.search_device(qb[:nq], dim, return_f64=True)
        oi, ok = _probe_expect(dec[:nq], cols)
        np.testing.assert_array_equal(I.cpu().numpy(), oi)
        np.testing.assert_array_equal(K.cpu().numpy(), ok)
    # one cosine batch over ordinary rows: bf16 queries == the same values handed over as fp32
    cs = _mk(gpu, "COSINE", dim)
    cs.add(synth.rows(0, 3000, dim, 9350))
    a = cs.search_device(qb, 10, return_f64=True)
    b = cs.search_device(qb.float(), 10, return_f64=True)
    for x, y, name in zip(a, b, ("D", "I", "K64")):
        assert torch.equal(x, y), f"cosine search, bf16 vs the same queries as fp32: {name} differs"


# ---- c. growth and reserve ---------------------------------------------------------------------------------------------------

GROW_OPS = [("add", 1000), ("reserve", 10), ("add", 24), ("add", 1), ("add", 511), ("add", 1), ("reserve", 5000), ("add", 700)]


@pytest.fixture(scope="module")
def grow_data():
    """2237 x 64 rows in six appends (the first capacity, 1024, filled exactly; then 1536, filled exactly; then 2304) with, in every
    append, near-duplicates of the queries that are nearer than those of the appends before: the answer changes at every step"""
    dim = 64
    sizes = [n for op, n in GROW_OPS if op == "add"]
    rows = synth.rows(0, sum(sizes), dim, 9400)
    q = synth.rows(0, 40, dim, 9401)
    lo = 0
    for s, size in enumerate(sizes):
        scale = np.float32(0.3 / (s + 1))
        for j in range(min(40, size)):
            jj = j if size > 1 else (s * 7) % 40
            rows[lo + (j * 13) % size] = q[jj] + scale * synth.rows(j, 1, dim, 9402 + s)[0]
        lo += size
    return rows, q


@pytest.mark.parametrize("f16", [False, True])
def test_growth_and_reserve_keep_rows_and_norms(gpu, grow_data, f16):
    """knn_realloc copies rows and |y|^2: after every append and every reserve the store reconstructs to the model bit for bit, and
    a 7-query and a 40-query L2 search return the oracle's ids and float64 keys over the MODEL rows"""
    import torch
    rows, q = grow_data
    dim, k = rows.shape[1], 5
    model = O.stored_rows(rows, "L2", f16).astype(np.float32)
    idx = _mk(gpu, "L2", dim, f16)
    qt = torch.from_numpy(q).to(gpu)
    n = 0
    for step, (op, arg) in enumerate(GROW_OPS):
        if op == "reserve":
            idx.reserve(arg)
        elif step % 2:
            idx.add(rows[n:n + arg]); n += arg
        else:
            idx.add_device(torch.from_numpy(rows[n:n + arg]).to(gpu)); n += arg
        what = f"after {op}({arg}), ntotal {n}, {'fp16' if f16 else 'fp32'} store"
        assert idx.ntotal == n
        _assert_bits(_held(idx, n, gpu), model[:n], f"{what}: reconstruct_batch")
        for nq in (7, 40):
            od, oi = O.knn(model[:n], q[:nq], k, "L2")
            assert O.rank_gaps(od).min() > 1e-6, "planted neighbours must separate the ranks"
            D, I, K = idx.search_device(qt[:nq], k, return_f64=True)
            np.testing.assert_array_equal(I.cpu().numpy(), oi, err_msg=f"{what}: ids of {nq} queries")
            np.testing.assert_allclose(K.cpu().numpy(), od, rtol=_key_rtol(dim), atol=0, err_msg=f"{what}: float64 keys of {nq} queries")
            assert torch.equal(D, K.float())
    assert n == len(rows)


def test_plane_is_rebuilt_after_growth(gpu, knn_oracle_lib):
    """a store that is full and has its f16 plane built grows by one row -- the nearest neighbour of query 0: the next certified scan
    reads a plane that holds it"""
    import torch
    from conftest import c_knn
    n, dim, nq, k = 20000, 64, 300, 10
    rows = synth.rows(0, n + 1, dim, 9450)
    q = synth.rows(0, nq, dim, 9451)
    for j in range(nq):
        rows[(j * 61 + 7) % n] = q[j] + np.float32(0.1) * synth.rows(j, 1, dim, 9452)[0]
    rows[n] = q[0] + np.float32(0.02) * synth.rows(0, 1, dim, 9453)[0]
    qt = torch.from_numpy(q).to(gpu)
    idx = _mk(gpu, "L2", dim)
    idx.add(rows[:n])                                    # one append: capacity == ntotal
    for m in (n, n + 1):
        if m > n:
            idx.add(rows[n:])
        D, I, K = idx.search_device(qt, k, return_f64=True)
        assert idx.last_launch()["scan_kind"] == "hi_tile" and idx.plane_info()["built"], (idx.last_launch(), idx.plane_info())
        _assert_bits(_held(idx, m, gpu), rows[:m], f"{m} rows")
        od, oi = c_knn(knn_oracle_lib, rows[:m], q, k, "L2")
        assert O.rank_gaps(od).min() > 1e-6
        np.testing.assert_array_equal(I.cpu().numpy(), oi)
        np.testing.assert_allclose(K.cpu().numpy(), od, rtol=_key_rtol(dim), atol=0)
    assert int(I[0, 0]) == n


# ---- d. snapshots, byte for byte ---------------------------------------------------------------------------------------------

def _read_snapshot(path):
    with open(path, "rb") as f:
        head = HEADER.unpack(f.read(HEADER.size))
        payload = np.fromfile(f, np.uint8)
    return head, payload


def _write_snapshot(path, stored, metric_id, version=2):
    """the snapshot layout written from numpy: version 2 as radad_knn_save writes it; version 1 has no dtype field and fp32 rows"""
    L = _lib()
    stored = np.ascontiguousarray(stored)
    n, dim = stored.shape
    with open(path, "wb") as f:
        f.write(b"RADADKNN" + struct.pack("<Iii", version, dim, metric_id))
        if version >= 2:
            f.write(struct.pack("<i", L.STORE_F16 if stored.dtype == np.float16 else L.STORE_F32))
        else:
            assert stored.dtype == np.float32
        f.write(struct.pack("<q", n))
        f.write(stored.tobytes())


N_BIG, ROW0, N_RANGE = 147456, 70001, 70003            # 75.5 MB = three 32 MiB stages; a range from inside the second into the third


@pytest.fixture(scope="module")
def big_rows():
    """147 456 x 128 synthetic rows, made once (the fp16 store's 256-wide rows are cut from them), and 300 queries per width with a
    near-duplicate each inside rows [ROW0, ROW0 + N_RANGE)"""
    base = synth.rows(0, N_BIG, 128, 9500)
    out = {}
    for dim in (128, 256):
        rows = base.copy() if dim == 128 else np.hstack([base, base[::-1] * np.float32(0.5)])
        q = synth.rows(0, 300, dim, 9501)
        for j in range(300):
            rows[ROW0 + (j * 211 + 5) % N_RANGE] = q[j] + np.float32(0.1) * synth.rows(j, 1, dim, 9502)[0]
        out[dim] = (rows, q)
    return out


@pytest.mark.parametrize("f16", [False, True])
def test_large_snapshot_bytes_ranges_and_add_against_load(gpu, big_rows, knn_oracle_lib, tmp_path, f16):
    """a store of three 32 MiB stages, saved after a growth (ntotal < capacity): the file is header + stored_rows().tobytes(); the
    whole file and two row ranges load back bit for bit; a search over a loaded range (|y|^2 from k_row_sqnorm) returns the C
    oracle's global ids; a loaded store and the store built by add answer alike"""
    import torch
    from conftest import c_knn
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex
    L = _lib()
    dim, k = (256, 10) if f16 else (128, 10)
    rows, q = big_rows[dim]
    model = O.stored_rows(rows, "L2", f16)
    model32 = model.astype(np.float32)
    assert model.nbytes == 75_497_472 and model.nbytes > 2 * (32 << 20)
    built = _mk(gpu, "L2", dim, f16)
    built.add_device(torch.from_numpy(rows[:100000]).to(gpu))
    built.add_device(torch.from_numpy(rows[100000:]).to(gpu))          # grows to 150 000 rows: 147 456 used
    path = str(tmp_path / "big.radad")
    built.save(path)
    head, payload = _read_snapshot(path)
    assert head == (b"RADADKNN", 2, dim, L.METRIC_L2, L.STORE_F16 if f16 else L.STORE_F32, N_BIG)
    assert payload.size == model.nbytes and os.path.getsize(path) == HEADER.size + model.nbytes
    assert np.array_equal(payload, model.reshape(-1).view(np.uint8)), "payload != stored_rows().tobytes()"
    del payload
    assert HipFlatIndex.snapshot_info(path) == {"d": dim, "metric": L.METRIC_L2, "store_f16": f16, "ntotal": N_BIG}
    # the whole file, and add against load
    loaded = _mk(gpu, "L2", dim, f16)
    loaded.load(path)
    assert loaded.ntotal == N_BIG
    _assert_bits(_held(loaded, N_BIG, gpu), model32, "whole-file load")
    qt = torch.from_numpy(q).to(gpu)
    for nq in (7, 300):
        a = built.search_device(qt[:nq], k, return_f64=True)
        b = loaded.search_device(qt[:nq], k, return_f64=True)
        for x, y, name in zip(a, b, ("D", "I", "K64")):
            assert torch.equal(x, y), f"{nq} queries, store built by add vs loaded store: {name} differs"
    del built, loaded
    # load(path, row0, n_rows)
    tail = _mk(gpu, "L2", dim, f16, id_base=N_BIG - 1)
    tail.load(path, N_BIG - 1, -1)
    assert tail.ntotal == 1
    _assert_bits(_held(tail, 1, gpu), model32[-1:], "range [ntotal - 1, ntotal)")
    part = _mk(gpu, "L2", dim, f16, id_base=ROW0)
    part.load(path, ROW0, N_RANGE)
    assert part.ntotal == N_RANGE
    want = model32[ROW0:ROW0 + N_RANGE]
    _assert_bits(_held(part, N_RANGE, gpu), want, f"range [{ROW0}, {ROW0 + N_RANGE})")
    D, I, K = part.search_device(qt, k, return_f64=True)
    assert part.last_launch()["scan_kind"] == "hi_tile", part.last_launch()
    I, K = I.cpu().numpy(), K.cpu().numpy()
    assert I.min() >= ROW0 and I.max() < ROW0 + N_RANGE
    sample = np.arange(0, 300, 13)[:24]
    od, oi = c_knn(knn_oracle_lib, want, q[sample], k, "L2", ROW0)
    assert O.rank_gaps(od).min() > 1e-6
    np.testing.assert_array_equal(I[sample], oi)
    np.testing.assert_allclose(K[sample], od, rtol=_key_rtol(dim), atol=0)
    np.testing.assert_array_equal(I[:, 0], ROW0 + (np.arange(300) * 211 + 5) % N_RANGE)


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
@pytest.mark.parametrize("f16", [False, True])
def test_small_snapshot_bytes(gpu, tmp_path, metric, f16):
    """one stage: 1500 x 100 rows saved after a growth (capacity 1536).  L2 / IP: payload == stored_rows().tobytes(); cosine: the
    payload is what reconstruct_batch returns (itself held to the model by the ingest test), in the store's dtype"""
    L = _lib()
    n, dim = 1500, 100
    rows = synth.rows(0, n, dim, 9600)
    rows[3] = np.resize(FP16_CASES, dim)
    rows[4] = 0
    idx = _mk(gpu, metric, dim, f16)
    idx.add(rows[:1000])
    idx.add(rows[1000:])
    path = str(tmp_path / "small.radad")
    idx.save(path)
    head, payload = _read_snapshot(path)
    assert head == (b"RADADKNN", 2, dim, idx.metric, L.STORE_F16 if f16 else L.STORE_F32, n)
    if metric == "COSINE":
        held = _held(idx, n, gpu)
        model = held.astype(np.float16) if f16 else held
        assert np.array_equal(model.astype(np.float32), held)
    else:
        model = O.stored_rows(rows, metric, f16)
    assert payload.tobytes() == model.tobytes(), "payload != the store's rows"
    again = _mk(gpu, metric, dim, f16)
    again.load(path)
    assert again.ntotal == n
    _assert_bits(_held(again, n, gpu), model.astype(np.float32), "load of the saved file")


def test_snapshots_written_on_the_host(gpu, tmp_path):
    """version 2 (fp32 and fp16) and version 1 (no dtype field, fp32 rows) files written from numpy load bit for bit, report the right
    header, and search like the oracle; a version 1 file is refused by an fp16 store"""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex
    L = _lib()
    n, dim, k = 3000, 64, 6
    rows = synth.rows(0, n, dim, 9650)
    q = synth.rows(0, 40, dim, 9651)
    for j in range(40):
        rows[(j * 71 + 3) % n] = q[j] + np.float32(0.2) * synth.rows(j, 1, dim, 9652)[0]
    qt = torch.from_numpy(q).to(gpu)
    for version, f16 in ((2, False), (2, True), (1, False)):
        stored = O.stored_rows(rows, "L2", f16)
        path = str(tmp_path / f"host_v{version}_{int(f16)}.radad")
        _write_snapshot(path, stored, L.METRIC_L2, version)
        assert os.path.getsize(path) == (32 if version == 2 else 28) + stored.nbytes
        assert HipFlatIndex.snapshot_info(path) == {"d": dim, "metric": L.METRIC_L2, "store_f16": f16, "ntotal": n}
        idx = _mk(gpu, "L2", dim, f16)
        idx.load(path)
        assert idx.ntotal == n
        model32 = stored.astype(np.float32)
        _assert_bits(_held(idx, n, gpu), model32, f"version {version} file")
        _assert_bits(idx.reconstruct(n - 1), model32[n - 1], f"version {version} file, reconstruct")
        od, oi = O.knn(model32, q, k, "L2")
        assert O.rank_gaps(od).min() > 1e-6
        for nq in (7, 40):
            D, I, K = idx.search_device(qt[:nq], k, return_f64=True)
            np.testing.assert_array_equal(I.cpu().numpy(), oi[:nq])
            np.testing.assert_allclose(K.cpu().numpy(), od[:nq], rtol=_key_rtol(dim), atol=0)
        if version == 1:
            with pytest.raises(OSError):
                _mk(gpu, "L2", dim, True).load(path)
            part = _mk(gpu, "L2", dim, False, id_base=17)
            part.load(path, 17, 1001)                              # the payload offset of a version 1 file is 28
            _assert_bits(_held(part, 1001, gpu), model32[17:1018], "range of a version 1 file")


# ---- e. IVF ------------------------------------------------------------------------------------------------------------------

def test_ivf_store_reconstructs_the_input_in_insertion_order(gpu, tmp_path):
    """list-major inside, insertion ids outside: after several adds reconstruct_batch(arange(n)) is the input, and again after
    save / load"""
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    dim, nlist = 64, 64
    sizes = [10000, 1, 16, 17, 2000]
    n = sum(sizes)
    rows = synth.rows(0, n, dim, 9700)
    ivf = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0)
    ivf.train(rows[:5000])
    lo = 0
    for s, size in enumerate(sizes):
        part = rows[lo:lo + size]
        ivf.add(torch.from_numpy(part).to(gpu) if s % 2 else part)
        lo += size
        assert ivf.ntotal == lo
        _assert_bits(ivf.reconstruct_batch(torch.arange(lo, device=gpu)).cpu().numpy(), rows[:lo], f"IVF store after {s + 1} adds")

    def check(index, what):
        assert index.ntotal == n
        ids = torch.cat([torch.arange(n, device=gpu), torch.tensor([-1, n, n + 7], device=gpu)])
        rec = index.reconstruct_batch(ids).cpu().numpy()
        _assert_bits(rec[:n], rows, what)
        assert not rec[n:].any(), f"{what}: ids -1 and >= ntotal must reconstruct to zeros"
        perm = torch.from_numpy(((np.arange(n, dtype=np.int64) * 7919) % n)).to(gpu)
        _assert_bits(index.reconstruct_batch(perm).cpu().numpy(), rows[perm.cpu().numpy()], f"{what}: permuted ids")
        _assert_bits(index.reconstruct(n - 1), rows[n - 1], f"{what}: reconstruct")

    check(ivf, "IVF store")
    assert len(np.unique(ivf.assignments())) > nlist // 2          # the rows really are spread over the lists
    path = str(tmp_path / "ivf.radad")
    ivf.save(path)
    head, payload = _read_snapshot(path)
    assert head == (b"RADADKNN", 2, dim, _lib().METRIC_L2, _lib().STORE_F32, n)
    assert payload.tobytes() == rows.tobytes(), "the IVF snapshot holds the rows in insertion order"
    back = R.HipIVFFlatIndex(dim, nlist, gpu.index or 0)
    back.load(path)
    check(back, "IVF store after save / load")
    np.testing.assert_array_equal(back.assignments(), ivf.assignments())
