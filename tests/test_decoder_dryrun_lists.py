"""CPU dry run of the list-column decode path.

Other kernels are recorded no-ops as in test_decoder_dryrun.py, but the
launchers the list path depends on — page decompression, the level decoder
and the two list kernels — are replaced by plain CPU references
(test_util/list_oracle.py, pyarrow / zlib codecs).  The decoder's Python
orchestration (page location, V1 level prefixes, level streams, bases,
summary, boundary) is therefore checked value for value against pyarrow
without a GPU; the kernels themselves are checked in test_gpu_lists.py.
"""
import zlib

import numpy as np
import pytest
import torch

from petastorm_amd import ops
from petastorm_amd.gpu.decoder import GpuRowGroupDecoder, ListColumn
from petastorm_amd.test_util.list_oracle import (assemble_lists_reference,
                                                 rle_hybrid_decode_reference)
from petastorm_amd.unischema import Unischema

pytestmark = pytest.mark.skipif(not ops.available(),
                                reason='HIP extension not built')

_LIST_KERNELS = ('list_count_batch', 'list_assemble_batch')


class _ListStubExt(object):
    """Host functions are real; kernel launchers are recorded.  The ones
    the list path reads results from run a CPU reference."""

    _NOOP = {'plain_fixed_decode_batch': (11,),
             'byte_array_offsets_batch': ()}

    def __init__(self):
        self._real = ops.ext()
        self.calls = []

    def __getattr__(self, name):
        if name in self._NOOP:
            def stub(*args):
                self.calls.append(name)
                for i in self._NOOP[name]:
                    args[i].zero_()
            return stub
        return getattr(self._real, name)

    def _codec(self, name, decompress, comp, start, end, out, out_off,
               out_len):
        self.calls.append(name)
        src, dst = comp.numpy(), out.numpy()
        for s, e, o, n in zip(start.tolist(), end.tolist(), out_off.tolist(),
                              out_len.tolist()):
            raw = decompress(src[s:e].tobytes(), n)
            assert len(raw) == n
            dst[o:o + n] = np.frombuffer(raw, dtype=np.uint8)

    def varlen_gather(self, src, src_off, lengths, dst, dst_off):
        self._codec('varlen_gather', lambda b, n: b, src, src_off,
                    src_off + lengths, dst, dst_off, lengths)

    def snappy_decompress_batch(self, comp, start, end, out, out_off,
                                out_len, status):
        import pyarrow as pa
        self._codec('snappy_decompress_batch',
                    lambda b, n: pa.decompress(b, n, codec='snappy',
                                               asbytes=True),
                    comp, start, end, out, out_off, out_len)

    def lz4_decompress_batch(self, comp, start, end, out, out_off, out_len,
                             status):
        import pyarrow as pa
        self._codec('lz4_decompress_batch',
                    lambda b, n: pa.decompress(b, n, codec='lz4_raw',
                                               asbytes=True),
                    comp, start, end, out, out_off, out_len)

    def inflate_batch(self, src, seg_off, seg_len, seg_first, seg_count,
                      dst, dst_off, dst_cap, produced, mode, status):
        assert mode == 2  # gzip members
        self._codec('inflate_batch',
                    lambda b, n: zlib.decompress(b, wbits=31),
                    src, seg_off, seg_off + seg_len, dst, dst_off, dst_cap)

    def rle_hybrid_decode_batch(self, data, start, end, bit_width, n_values,
                                out_off, out, status):
        self.calls.append('rle_hybrid_decode_batch')
        buf = data.numpy()
        for s, e, bw, n, o in zip(start.tolist(), end.tolist(),
                                  bit_width.tolist(), n_values.tolist(),
                                  out_off.tolist()):
            out[o:o + n] = torch.from_numpy(
                rle_hybrid_decode_reference(buf, s, e, bw, n))

    def list_count_batch(self, rep, dfl, n_entries, entry0, def_slot,
                         max_def, counts):
        self.calls.append('list_count_batch')
        for p, (n, e0) in enumerate(zip(n_entries.tolist(),
                                        entry0.tolist())):
            r, d = rep[e0:e0 + n], dfl[e0:e0 + n]
            counts[p, 0] = int((r == 0).sum())
            counts[p, 1] = int((d >= def_slot).sum())
            counts[p, 2] = int((d == max_def).sum())

    def list_assemble_batch(self, rep, dfl, n_entries, entry0, bases,
                            val_buf, val_start, val_end, esize, fill,
                            def_slot, max_def, list_nullable, values,
                            offsets, list_valid, elem_valid, status):
        self.calls.append('list_assemble_batch')
        ref = assemble_lists_reference(
            rep.numpy(), dfl.numpy(), n_entries.numpy(), val_buf.numpy(),
            val_start.numpy(), val_end.numpy(), esize, fill, def_slot,
            max_def, list_nullable, offsets.numel() - 1)
        # the bases the decoder derived must be the exclusive scan
        excl = np.cumsum(ref['counts'], 0) - ref['counts']
        np.testing.assert_array_equal(bases.numpy(), excl)
        slots = len(ref['elem_valid'])
        values[:slots * esize] = torch.from_numpy(ref['values'])
        elem_valid[:slots] = torch.from_numpy(ref['elem_valid'])
        offsets.copy_(torch.from_numpy(ref['offsets']))
        list_valid.copy_(torch.from_numpy(ref['list_valid']))
        status.copy_(torch.from_numpy(ref['status']))


@pytest.fixture()
def stub_decoder():
    dec = GpuRowGroupDecoder('cpu')
    dec._ext = _ListStubExt()
    return dec, dec._ext


def _decode_file(dec, path, columns, rg=0):
    import pyarrow.parquet as pq
    pf = pq.ParquetFile(path)
    schema = Unischema.from_arrow_schema(pf.schema_arrow)
    host, meta = dec.read_rowgroup_bytes(path, pf.metadata, pf.schema, rg,
                                         columns)
    out, _ = dec.decode(host, meta, schema)
    dec.flush_status()
    return out, schema, pf


_CODEC_KERNEL = {'snappy': ['snappy_decompress_batch'],
                 'gzip': ['inflate_batch'], 'lz4': ['lz4_decompress_batch']}
_LIST_SEQ = ['rle_hybrid_decode_batch', 'list_count_batch',
             'list_assemble_batch']


@pytest.mark.parametrize('compression', ['none', 'snappy', 'gzip', 'lz4',
                                         'zstd'])
@pytest.mark.parametrize('version', ['1.0', '2.0'])
def test_dryrun_plain_lists_native(stub_decoder, tmp_path, version,
                                   compression):
    """A PLAIN list store: exact launch order, ListColumn results equal to
    pyarrow's, nothing on the assist until the boundary meets ragnull's null
    elements."""
    from petastorm_amd.test_util.dataset_gen import create_list_dataset
    dec, stub = stub_decoder
    create_list_dataset('file://' + str(tmp_path), version, compression,
                        num_rows=150, rowgroup_size=100)
    names = ['id', 'rag', 'fix', 'req', 'ragnull']
    for rg in (0, 1):  # 100 rows, then the 50-row remainder
        del stub.calls[:]
        out, schema, pf = _decode_file(dec, str(tmp_path / 'data.parquet'),
                                       names, rg)
        codec = _CODEC_KERNEL.get(compression, [])
        if version == '1.0':
            assert stub.calls == codec + ['plain_fixed_decode_batch'] + \
                (codec + _LIST_SEQ) * 4
        else:
            # a V2 writer leaves a page uncompressed where compression does
            # not shrink it: the codec kernel runs for the chunks that have
            # a compressed page, ahead of the list sequence, and raw pages
            # of such a chunk are gathered in next to them
            rest = [c for c in stub.calls
                    if c not in codec + ['varlen_gather']]
            assert rest == ['plain_fixed_decode_batch'] + _LIST_SEQ * 4
            if codec:
                assert codec[0] in stub.calls
                assert all(c not in codec or stub.calls[i + 1] in
                           ('varlen_gather', 'rle_hybrid_decode_batch',
                            'plain_fixed_decode_batch')
                           for i, c in enumerate(stub.calls))
        assert not dec.cpu_assist_columns
        truth = pf.read_row_group(rg).to_pydict()
        n = len(truth['id'])
        for name in names[1:]:
            col = out[name]
            assert isinstance(col, ListColumn) and len(col) == n
            want = truth[name]
            lens = [len(v) for v in want if v is not None]
            null_elems = sum(e is None for v in want if v is not None
                             for e in v)
            assert col.summary == (
                n, sum(v is None for v in want), null_elems,
                min(lens + [0] if None in want else lens),
                max(lens))
            off = col.offsets.numpy()
            vals = col.values.numpy()
            assert vals.dtype == np.dtype(schema.fields[name].numpy_dtype)
            ev = col.elem_valid.numpy() if col.elem_valid is not None \
                else np.ones(len(vals), bool)
            got = [None if col.list_valid is not None and
                   not col.list_valid[i] else
                   [v if ok else None for v, ok in
                    zip(vals[off[i]:off[i + 1]].tolist(),
                        ev[off[i]:off[i + 1]].tolist())]
                   for i in range(n)]
            assert got == want, name

        # boundary: dense tensors, per-row arrays, assist
        fix = dec.decode_list_column(out['fix'], schema.fields['fix'])
        assert fix.dtype == torch.int32 and fix.shape == (n, 9)
        assert fix.tolist() == truth['fix']
        req = dec.decode_list_column(out['req'], schema.fields['req'])
        assert req.dtype == torch.int64 and req.tolist() == truth['req']
        rag = dec.decode_list_column(out['rag'], schema.fields['rag'])
        assert rag.dtype == object and len(rag) == n
        for g, w in zip(rag, truth['rag']):
            if w is None:
                assert g is None
            else:
                assert g.dtype == np.float32 and g.tolist() == w
        assert not dec.cpu_assist_columns
        assert dec.decode_list_column(out['ragnull'],
                                      schema.fields['ragnull']) is None
        assert dec.cpu_assist_columns == {'ragnull'}
        dec.cpu_assist_columns.clear()


def _write(tmp_path, table, **kw):
    import pyarrow.parquet as pq
    path = str(tmp_path / 'p.parquet')
    pq.write_table(table, path, compression='none', **kw)
    return path


def _out_of_scope_tables():
    import pyarrow as pa
    ints = [[1, 2], [], [3]] * 20
    return {
        'dictionary': (pa.table({'c': pa.array(ints, pa.list_(pa.int32()))}),
                       dict(use_dictionary=True)),
        'list_of_string': (
            pa.table({'c': pa.array([['a', 'bc'], [], ['d']] * 20,
                                    pa.list_(pa.string()))}),
            dict(use_dictionary=False)),
        'list_of_list': (
            pa.table({'c': pa.array([[[1], [2, 3]], [], [[4]]] * 20,
                                    pa.list_(pa.list_(pa.int32())))}),
            dict(use_dictionary=False)),
        'struct_with_list': (
            pa.table({'c': pa.array(
                [{'l': v} for v in ints],
                pa.struct([('l', pa.list_(pa.int32()))]))}),
            dict(use_dictionary=False)),
        'list_of_timestamp': (
            pa.table({'c': pa.array([[1, 2], [], [3]] * 20,
                                    pa.list_(pa.timestamp('us')))}),
            dict(use_dictionary=False)),
    }


@pytest.mark.filterwarnings('ignore:Column')
@pytest.mark.parametrize('case', ['dictionary', 'list_of_string',
                                  'list_of_list', 'struct_with_list',
                                  'list_of_timestamp'])
def test_dryrun_out_of_scope_lists_take_assist(stub_decoder, tmp_path, case):
    """Outside the native scope the chunk returns the marker as before and
    no list launcher runs."""
    dec, stub = stub_decoder
    table, kw = _out_of_scope_tables()[case]
    out, _, _ = _decode_file(dec, _write(tmp_path, table, **kw), ['c'])
    assert out['c'] is None
    assert dec.cpu_assist_columns == {'c'}
    assert not set(stub.calls) & set(_LIST_KERNELS)


def test_dryrun_narrow_and_unsigned_list_elements(stub_decoder, tmp_path):
    """uint8 / int16 / uint32 elements are stored as INT32: ragged rows come
    back in the logical dtype, as on the CPU route."""
    import pyarrow as pa
    dec, stub = stub_decoder
    rows = [[250, 3], [], [7, 8, 255]] * 10
    big = [[4000000000, 3], [], [7, 8, 9]] * 10
    table = pa.table({'u8': pa.array(rows, pa.list_(pa.uint8())),
                      'i16': pa.array(rows, pa.list_(pa.int16())),
                      'u32': pa.array(big, pa.list_(pa.uint32()))})
    out, schema, _ = _decode_file(
        dec, _write(tmp_path, table, use_dictionary=False),
        ['u8', 'i16', 'u32'])
    for name, dt, want in (('u8', np.uint8, rows), ('i16', np.int16, rows),
                           ('u32', np.uint32, big)):
        got = dec.decode_list_column(out[name], schema.fields[name])
        assert [g.tolist() for g in got] == want
        assert all(g.dtype == dt for g in got)
    assert not dec.cpu_assist_columns


def test_dryrun_truncated_levels_raise(stub_decoder, tmp_path):
    """Levels that start fewer rows than the row group holds raise the
    decode error instead of returning a short column."""
    from petastorm_amd.test_util.dataset_gen import create_list_dataset
    dec, stub = stub_decoder
    create_list_dataset('file://' + str(tmp_path), '1.0', 'none',
                        num_rows=60)
    real = stub.list_count_batch

    def short(rep, dfl, n_entries, entry0, def_slot, max_def, counts):
        rep[0] = 1  # the first row now continues a list that never began
        real(rep, dfl, n_entries, entry0, def_slot, max_def, counts)
    stub.list_count_batch = short
    with pytest.raises(RuntimeError, match='GPU decode error in list:fix'):
        _decode_file(dec, str(tmp_path / 'data.parquet'), ['fix'])
