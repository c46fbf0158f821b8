"""List columns on the GPU route: the two list kernels against a numpy
oracle, their status codes, and PLAIN list stores end to end.

Every comparison is exact — the path only copies bytes.  Ground truth is
pyarrow on the CPU (``to_pylist``) or the numpy reference assembler in
test_util/list_oracle.py, never other GPU output.  All tests need an MI355X.
"""
import numpy as np
import pytest
import torch

from petastorm_amd import ops
from petastorm_amd.test_util.list_oracle import assemble_lists_reference

pytestmark = pytest.mark.gpu

_GUARD = 64        # sentinel bytes / entries placed after every output
_NAN32 = 0x7FC00000
_NAN64 = 0x7FF8000000000000


@pytest.fixture(scope='module')
def ext():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    return ops.ext()


# ---------------------------------------------------------------------------
# 1. kernels vs the numpy oracle
# ---------------------------------------------------------------------------

def _levels(rows, list_nullable, elem_nullable):
    """Python rows (None | list of value-or-None) -> (rep, def, values in
    storage order), per the Parquet three-level list layout."""
    max_def = 1 + list_nullable + elem_nullable
    rep, dfl, vals = [], [], []
    for row in rows:
        if row is None:
            assert list_nullable
            rep.append(0), dfl.append(0)
        elif not row:
            rep.append(0), dfl.append(1 if list_nullable else 0)
        else:
            for j, v in enumerate(row):
                rep.append(1 if j else 0)
                if v is None:
                    assert elem_nullable
                    dfl.append(max_def - 1)
                else:
                    dfl.append(max_def)
                    vals.append(v)
    return (np.asarray(rep, np.int32), np.asarray(dfl, np.int32), vals,
            max_def)


def _random_rows(rng, lens, list_nullable, elem_nullable):
    rows = []
    for i, k in enumerate(lens):
        if list_nullable and k == 0 and i % 2:
            rows.append(None)
            continue
        rows.append([None if elem_nullable and rng.rand() < 0.25
                     else int(rng.randint(1, 1 << 30)) for _ in range(k)])
    return rows


def _layouts():
    """name -> (row lengths, entries per page).  An empty or null list is
    one entry; a list of k elements is k entries."""
    # 20 lists of 3 = 60 entries, then one of 8 covering entries 60..67
    cross = [3] * 20 + [8] + [0, 1, 2, 5, 0, 3, 4] * 3 + [5, 5, 1]
    assert sum(max(1, k) for k in cross) == 130
    # 175 entries; the list of 9 covers entries 66..74 and so continues
    # from page 0 (70 entries) into page 1; page 2 starts inside a list too
    three = [2] * 33 + [9] + [4] * 25
    assert sum(three) == 175
    return {
        'one_entry': ([1], [1]),
        'cross_64': (cross, [130]),
        'three_pages': (three, [70, 67, 38]),
        'all_empty': ([0] * 150, [100, 50]),
    }


def _run_kernels(ext, rep, dfl, page_nval, page_vals, esize, fill, def_slot,
                 max_def, list_nullable, n_rows, short_page=None):
    """Launch list_count_batch, the device cumsum and list_assemble_batch.
    Value spans sit at odd offsets in ``val_buf``.  Every output is a view
    into a larger sentinel-filled buffer, so a write past its end shows."""
    dev = 'cuda'
    np_dt = np.int32 if esize == 4 else np.int64
    chunks, val_start, val_end, pos = [], [], [], 0
    for vals in page_vals:
        pad = 3 if esize == 4 else 5   # unaligned value spans
        chunks.append(np.full(pad, 0xEE, np.uint8))
        raw = np.asarray(vals, dtype=np_dt).view(np.uint8)
        chunks.append(raw)
        val_start.append(pos + pad)
        val_end.append(pos + pad + len(raw))
        pos += pad + len(raw)
    chunks.append(np.full(16, 0xEE, np.uint8))
    val_buf = np.concatenate(chunks)
    val_start = np.asarray(val_start, np.int64)
    val_end = np.asarray(val_end, np.int64)
    if short_page is not None:
        val_end[short_page] -= esize   # declared one element short
    page_nval = np.asarray(page_nval, np.int32)
    entry0 = np.concatenate([[0], np.cumsum(page_nval)[:-1]]) \
        .astype(np.int64)
    total, n_pages = int(page_nval.sum()), len(page_nval)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def guarded(n, dtype):
        big = torch.full((n + _GUARD,), 0x5A, dtype=dtype, device=dev)
        return big, big[:n]

    rep_d, dfl_d = t(rep), t(dfl)
    n_ent, e0 = t(page_nval), t(entry0)
    counts = torch.empty((n_pages, 3), dtype=torch.int64, device=dev)
    ext.list_count_batch(rep_d, dfl_d, n_ent, e0, def_slot, max_def, counts)
    bases = torch.cumsum(counts, 0) - counts
    values_big, values = guarded(total * esize, torch.uint8)
    offsets_big, offsets = guarded(n_rows + 1, torch.int64)
    lvalid_big, lvalid = guarded(n_rows, torch.uint8)
    evalid_big, evalid = guarded(total, torch.uint8)
    status = torch.zeros(n_pages, dtype=torch.int32, device=dev)
    ext.list_assemble_batch(
        rep_d, dfl_d, n_ent, e0, bases, t(val_buf), t(val_start),
        t(val_end), esize, fill, def_slot, max_def, list_nullable, values,
        offsets, lvalid, evalid, status)
    torch.cuda.synchronize()
    got = dict(counts=counts.cpu().numpy(), offsets=offsets.cpu().numpy(),
               values=values.cpu().numpy(), elem_valid=evalid.cpu().numpy(),
               list_valid=lvalid.cpu().numpy(),
               status=status.cpu().numpy())
    guards = dict(values=values_big[total * esize:],
                  offsets=offsets_big[n_rows + 1:],
                  list_valid=lvalid_big[n_rows:], elem_valid=evalid_big[total:])
    for name, g in guards.items():
        assert bool((g == 0x5A).all()), 'write past the end of ' + name
    want = assemble_lists_reference(
        rep, dfl, page_nval, val_buf, val_start, val_end, esize, fill,
        def_slot, max_def, list_nullable, n_rows)
    return got, want


def _case(layout, list_nullable, elem_nullable, esize):
    rng = np.random.RandomState(7)
    lens, page_nval = _layouts()[layout]
    rows = _random_rows(rng, lens, list_nullable, elem_nullable)
    rep, dfl, vals, max_def = _levels(rows, list_nullable, elem_nullable)
    assert len(rep) == sum(page_nval)
    if esize == 8:
        vals = [(v << 31) | 5 for v in vals]
    page_vals, e, v = [], 0, 0
    for n in page_nval:   # stored values of each page, in order
        k = int((dfl[e:e + n] == max_def).sum())
        page_vals.append(vals[v:v + k])
        e, v = e + n, v + k
    return rows, rep, dfl, page_nval, page_vals, max_def


@pytest.mark.parametrize('esize', [4, 8])
@pytest.mark.parametrize('list_nullable,elem_nullable',
                         [(False, False), (True, False), (False, True),
                          (True, True)])   # max_def 1, 2, 2, 3
@pytest.mark.parametrize('layout', ['one_entry', 'cross_64', 'three_pages',
                                    'all_empty'])
def test_list_kernels_match_numpy_oracle(ext, layout, list_nullable,
                                         elem_nullable, esize):
    rows, rep, dfl, page_nval, page_vals, max_def = _case(
        layout, list_nullable, elem_nullable, esize)
    if layout == 'cross_64':
        starts = np.flatnonzero(rep == 0)
        assert ((starts[:-1] < 63) & (starts[1:] > 64)).any()
    if layout == 'three_pages':
        assert rep[70] == 1 and rep[137] == 1   # pages 1, 2 start mid-list
    fill = _NAN32 if esize == 4 else _NAN64
    def_slot = max_def - (1 if elem_nullable else 0)
    got, want = _run_kernels(ext, rep, dfl, page_nval, page_vals, esize,
                             fill, def_slot, max_def, list_nullable,
                             len(rows))
    assert want['status'].tolist() == [0] * len(page_nval)
    np.testing.assert_array_equal(got['status'], want['status'])
    np.testing.assert_array_equal(got['counts'], want['counts'])
    np.testing.assert_array_equal(got['offsets'], want['offsets'])
    np.testing.assert_array_equal(got['list_valid'], want['list_valid'])
    slots = int(want['offsets'][-1])
    assert slots == sum(len(r) for r in rows if r)
    np.testing.assert_array_equal(got['elem_valid'][:slots],
                                  want['elem_valid'])
    np.testing.assert_array_equal(got['values'][:slots * esize],
                                  want['values'])
    # and the oracle itself agrees with the rows it was built from
    np_dt = np.int32 if esize == 4 else np.int64
    flat = want['values'].view(np_dt)
    off = want['offsets']
    stored = iter(v for vals in page_vals for v in vals)
    for i, row in enumerate(rows):
        if row is None:
            assert not want['list_valid'][i] and off[i + 1] == off[i]
            continue
        assert want['list_valid'][i] and off[i + 1] - off[i] == len(row)
        for j, v in enumerate(row):
            assert want['elem_valid'][off[i] + j] == (v is not None)
            if v is not None:
                assert flat[off[i] + j] == next(stored)


# ---------------------------------------------------------------------------
# 2. corrupt input gives a status code, never an access out of bounds
# ---------------------------------------------------------------------------

def _status_case():
    rows, rep, dfl, page_nval, page_vals, max_def = _case(
        'three_pages', True, True, 4)
    return rows, rep, dfl, page_nval, page_vals, max_def


def test_short_value_span_sets_status_3(ext):
    """Page 1's value span is declared one element short: the kernel checks
    the span before it reads, skips that value and reports code 3.  The
    sentinels after every output stay untouched (_run_kernels)."""
    rows, rep, dfl, page_nval, page_vals, max_def = _status_case()
    got, want = _run_kernels(ext, rep, dfl, page_nval, page_vals, 4, _NAN32,
                             max_def - 1, max_def, True, len(rows),
                             short_page=1)
    assert want['status'].tolist() == [0, 3, 0]
    assert got['status'].tolist() == [0, 3, 0]
    np.testing.assert_array_equal(got['offsets'], want['offsets'])
    np.testing.assert_array_equal(got['counts'], want['counts'])


def test_first_entry_continuing_a_row_sets_status_1(ext):
    rows, rep, dfl, page_nval, page_vals, max_def = _status_case()
    rep = rep.copy()
    rep[0] = 1
    got, want = _run_kernels(ext, rep, dfl, page_nval, page_vals, 4, _NAN32,
                             max_def - 1, max_def, True, len(rows))
    assert want['status'].tolist() == [1, 0, 0]
    assert got['status'].tolist() == [1, 0, 0]
    assert got['counts'][:, 0].sum() == len(rows) - 1


def test_more_rows_than_the_row_group_sets_status_2(ext):
    """Levels that start more rows than ``offsets`` has room for: the extra
    row is reported (code 2) and not written."""
    rows, rep, dfl, page_nval, page_vals, max_def = _status_case()
    got, want = _run_kernels(ext, rep, dfl, page_nval, page_vals, 4, _NAN32,
                             max_def - 1, max_def, True, len(rows) - 1)
    assert want['status'].tolist() == [0, 0, 2]
    assert got['status'].tolist() == [0, 0, 2]
    np.testing.assert_array_equal(got['offsets'], want['offsets'])


# ---------------------------------------------------------------------------
# 3 + 4. end to end, and parity with the CPU route
# ---------------------------------------------------------------------------

_N_ROWS, _RG = 300, 150


@pytest.fixture(scope='module')
def list_store(tmp_path_factory):
    """(version, compression) -> (url, pyarrow ground truth per column),
    each store written and read back by pyarrow once per module."""
    from petastorm_amd.test_util.dataset_gen import create_list_dataset
    cache = {}

    def get(version, compression):
        key = (version, compression)
        if key not in cache:
            import pyarrow.parquet as pq
            path = tmp_path_factory.mktemp(
                'lists_{}_{}'.format(version[0], compression))
            url = 'file://' + str(path)
            create_list_dataset(url, version, compression, num_rows=_N_ROWS,
                                rowgroup_size=_RG)
            pf = pq.ParquetFile(str(path / 'data.parquet'))
            assert pf.metadata.num_row_groups == 2
            truth = [pf.read_row_group(rg).to_pydict() for rg in (0, 1)]
            cache[key] = (url, str(path / 'data.parquet'), truth)
        return cache[key]
    return get


def _read(url, device):
    from petastorm_amd import make_batch_reader
    kwargs = {'device': device} if device else {}
    with make_batch_reader(url, shuffle_row_groups=False, **kwargs) as r:
        batches = list(r)
        diag = r.diagnostics if device else None
    # the CPU route's worker pool may deliver row groups out of order
    batches.sort(key=lambda b: int(b.id[0]))
    return batches, diag


def _assert_ragged_equal(got, want, name):
    assert isinstance(got, np.ndarray) and got.dtype == object
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, (name, i)
        else:
            assert isinstance(g, np.ndarray) and g.dtype == np.float32, \
                (name, i)
            assert g.tolist() == w, (name, i)


@pytest.mark.parametrize('version,compression', [
    ('1.0', 'none'), ('1.0', 'snappy'), ('2.0', 'none'), ('2.0', 'snappy'),
    ('1.0', 'zstd'), ('2.0', 'lz4')])
def test_list_store_end_to_end(ext, list_store, version, compression):
    from petastorm_amd.workers.batch_worker import arrow_table_to_numpy_dict
    import pyarrow.parquet as pq
    url, path, truth = list_store(version, compression)
    batches, diag = _read(url, 'cuda')
    assert len(batches) == 2
    pf = pq.ParquetFile(path)
    for rg, (b, want) in enumerate(zip(batches, truth)):
        n = len(want['id'])
        assert b.id.is_cuda and b.id.cpu().tolist() == want['id']
        assert b.fix.is_cuda and b.fix.dtype == torch.int32
        assert tuple(b.fix.shape) == (n, 9)
        assert b.fix.cpu().tolist() == want['fix']
        assert b.req.is_cuda and b.req.dtype == torch.int64
        assert tuple(b.req.shape) == (n, 9)
        assert b.req.cpu().tolist() == want['req']
        _assert_ragged_equal(b.rag, want['rag'], 'rag')
        # ragnull has null elements: it still goes through the assist and
        # returns what the assist returns
        assist = arrow_table_to_numpy_dict(
            pf.read_row_group(rg, columns=['ragnull']), None)['ragnull']
        assert len(b.ragnull) == n
        for i, (g, w) in enumerate(zip(b.ragnull, assist)):
            if w is None:
                assert g is None, i
            else:
                assert g.dtype == w.dtype
                np.testing.assert_array_equal(g, w)
    assert diag['cpu_assist_columns'] == ['ragnull']


def test_list_columns_match_cpu_route(ext, list_store):
    url, _, truth = list_store('1.0', 'snappy')
    gpu, _ = _read(url, 'cuda')
    cpu, _ = _read(url, None)
    assert len(gpu) == len(cpu) == 2
    for g, c in zip(gpu, cpu):
        for name in ('fix', 'req'):
            gv, cv = getattr(g, name).cpu().numpy(), getattr(c, name)
            assert gv.dtype == cv.dtype and gv.shape == cv.shape
            np.testing.assert_array_equal(gv, cv)
        assert len(g.rag) == len(c.rag) and c.rag.dtype == object
        for i, (gv, cv) in enumerate(zip(g.rag, c.rag)):
            if cv is None:
                assert gv is None, i
            else:
                assert gv.dtype == cv.dtype
                np.testing.assert_array_equal(gv, cv)
