"""CPU dry-run of the GPU decoder's Python orchestration.

Device kernels are stubbed to no-ops (device='cpu'); the host-side pieces
(page walk, offset scans, jpeg/png parse) are the real native functions.
This exercises every code path of GpuRowGroupDecoder.decode() so pure-Python
regressions (unbound names, wrong shapes, bad offsets math) are caught
without a GPU.
"""
import numpy as np
import pytest
import torch

from petastorm_amd import ops
from petastorm_amd.etl import dataset_metadata as dsm
from petastorm_amd.fs_utils import get_filesystem_and_path_or_paths
from petastorm_amd.gpu.decoder import ByteArrayColumn, GpuRowGroupDecoder

pytestmark = pytest.mark.skipif(not ops.available(),
                                reason='HIP extension not built')


class _StubExt(object):
    """Host functions are real; kernel launchers are recorded no-ops."""

    _KERNELS = {'snappy_decompress_batch', 'rle_hybrid_decode_batch',
                'byte_array_offsets_batch', 'varlen_gather',
                'npy_payload_offsets', 'plain_fixed_decode_batch',
                'nhwc_to_nchw_normalize', 'jpeg_decode_batch',
                'lz4_decompress_batch',
                'inflate_batch', 'png_unfilter_batch', 'bswap16',
                'delta_binary_packed_batch',
                'delta_length_byte_array_batch',
                'delta_byte_array_lengths_batch',
                'delta_byte_array_reconstruct_batch',
                'byte_stream_split_batch', 'bool_unpack_batch'}

    def __init__(self):
        self._real = ops.ext()
        self.calls = []

    # output-tensor positions per kernel whose results feed HOST-side
    # indexing later (a no-op stub would leave uninitialized memory there,
    # making the dry run flaky on heap reuse)
    _OUTPUTS = {'rle_hybrid_decode_batch': (6,),
                'plain_fixed_decode_batch': (11,),
                'varlen_gather': (3,),
                'delta_byte_array_lengths_batch': (5, 6, 7),
                # decompressed pages: the V1 level-length prefix of a
                # nullable column is read back from this buffer
                'snappy_decompress_batch': (3,),
                'lz4_decompress_batch': (3,),
                'inflate_batch': (5,)}

    def __getattr__(self, name):
        if name in self._KERNELS:
            outs = self._OUTPUTS.get(name, ())
            def stub(*args, **kwargs):
                self.calls.append(name)
                for i in outs:
                    if i < len(args) and isinstance(args[i], torch.Tensor):
                        args[i].zero_()
            return stub
        return getattr(self._real, name)


def _seq(spec):
    return [{'snappy': 'snappy_decompress_batch',
             'lz4': 'lz4_decompress_batch',
             'fixed': 'plain_fixed_decode_batch',
             'ba_offsets': 'byte_array_offsets_batch',
             'rle': 'rle_hybrid_decode_batch',
             'npy': 'npy_payload_offsets'}.get(k, k) for k in spec.split()]


# exact ordered kernel launches per dry-run store
_SEQ = {
    'scalar_none': _seq('fixed fixed fixed'),
    'scalar_snappy': _seq('snappy fixed snappy fixed snappy fixed'),
    'scalar_gzip': _seq('inflate_batch fixed inflate_batch fixed '
                        'inflate_batch fixed'),
    'lz4_scalar': _seq('lz4 fixed lz4 fixed'),
    'imagenet': _seq('snappy fixed jpeg_decode_batch'),
    'sequence': _seq('snappy fixed snappy ba_offsets npy varlen_gather'),
    'png': _seq('snappy fixed inflate_batch png_unfilter_batch'),
    'compressed_ndarray': _seq('snappy fixed inflate_batch npy '
                               'varlen_gather'),
    'npz': _seq('snappy fixed snappy ba_offsets inflate_batch npy '
                'varlen_gather'),
    'dictionary': _seq('rle varlen_gather rle'),
    'delta': _seq('delta_binary_packed_batch '
                  'delta_length_byte_array_batch'),
    'bool_bss_delta_ba': _seq('byte_stream_split_batch bool_unpack_batch '
                              'delta_byte_array_lengths_batch '
                              'delta_byte_array_reconstruct_batch'),
}


@pytest.fixture()
def stub_decoder(monkeypatch):
    dec = GpuRowGroupDecoder('cpu')
    stub = _StubExt()
    dec._ext = stub
    return dec, stub


def _decode_all(dec, url, columns):
    import pyarrow.parquet as pq
    fs, path = get_filesystem_and_path_or_paths(url)
    pieces = dsm.load_row_groups(fs, path)
    schema, _ = dsm.infer_or_load_unischema(fs, path)
    piece = pieces[0]
    pf = pq.ParquetFile(piece.path)
    host, meta = dec.read_rowgroup_bytes(piece.path, pf.metadata, pf.schema,
                                         piece.row_group, columns)
    out, _ = dec.decode(host, meta, schema)
    dec.flush_status()
    return out, schema


@pytest.mark.parametrize('compression', ['snappy', 'none', 'gzip'])
def test_dryrun_scalar_paths(stub_decoder, tmp_path, compression):
    from petastorm_amd.test_util.dataset_gen import create_scalar_dataset
    dec, stub = stub_decoder
    url = 'file://' + str(tmp_path / ('s_' + compression))
    create_scalar_dataset(url, num_rows=500, rowgroup_size=200,
                          compression=compression)
    out, _ = _decode_all(dec, url, ['id', 'f0', 'i1'])
    assert set(out) == {'id', 'f0', 'i1'}
    assert 'plain_fixed_decode_batch' in stub.calls
    if compression == 'snappy':
        assert 'snappy_decompress_batch' in stub.calls
    assert stub.calls == _SEQ['scalar_' + compression]


def test_dryrun_imagenet_paths(stub_decoder, tmp_path):
    from petastorm_amd.test_util.dataset_gen import create_imagenet_dataset
    dec, stub = stub_decoder
    url = 'file://' + str(tmp_path / 'im')
    create_imagenet_dataset(url, num_rows=8, rowgroup_size_mb=8)
    out, schema = _decode_all(dec, url, ['image', 'label'])
    col = out['image']
    assert isinstance(col, ByteArrayColumn)
    assert col.jpeg_meta is not None  # prepare_host parsed the headers
    decoded = dec.decode_jpeg_column(col, schema.fields['image'])
    assert decoded is not None and decoded.shape == (8, 224, 224, 3)
    assert 'jpeg_decode_batch' in stub.calls
    assert stub.calls == _SEQ['imagenet']


def test_dryrun_sequence_and_png_paths(stub_decoder, tmp_path):
    from petastorm_amd.test_util.dataset_gen import (
        create_hello_world_dataset, create_sequence_dataset)
    dec, stub = stub_decoder
    url = 'file://' + str(tmp_path / 'seq')
    create_sequence_dataset(url, num_rows=30, rowgroup_size_mb=0.5)
    out, schema = _decode_all(dec, url, ['timestamp', 'tokens'])
    decoded = dec.decode_ndarray_column(out['tokens'],
                                        schema.fields['tokens'])
    assert decoded.shape == (30, 1024)
    assert 'npy_payload_offsets' in stub.calls
    assert stub.calls == _SEQ['sequence']

    url2 = 'file://' + str(tmp_path / 'hw')
    create_hello_world_dataset(url2, num_rows=4, rowgroup_size_mb=4)
    out2, schema2 = _decode_all(dec, url2, ['id', 'image1'])
    png = dec.decode_png_column(out2['image1'], schema2.fields['image1'])
    assert png is not None and png.shape == (4, 128, 256, 3)
    assert 'inflate_batch' in stub.calls
    assert 'png_unfilter_batch' in stub.calls
    assert stub.calls == _SEQ['sequence'] + _SEQ['png']


def test_dryrun_compressed_ndarray(stub_decoder, tmp_path):
    from petastorm_amd.codecs import CompressedNdarrayCodec, ScalarCodec
    from petastorm_amd.etl.dataset_metadata import materialize_dataset
    from petastorm_amd.unischema import Unischema, UnischemaField
    dec, stub = stub_decoder
    schema = Unischema('Z', [
        UnischemaField('id', np.int64, (), ScalarCodec(), False),
        UnischemaField('mat', np.float32, (8, 4), CompressedNdarrayCodec(),
                       False)])
    url = 'file://' + str(tmp_path / 'z')
    rng = np.random.RandomState(0)
    with materialize_dataset(url, schema, 1) as w:
        w.write_rows([{'id': np.int64(i),
                       'mat': rng.rand(8, 4).astype(np.float32)}
                      for i in range(20)])
    out, sch = _decode_all(dec, url, ['id', 'mat'])
    z = dec.decode_compressed_ndarray_column(out['mat'], sch.fields['mat'])
    assert z.shape == (20, 8, 4)
    assert 'inflate_batch' in stub.calls
    assert stub.calls == _SEQ['compressed_ndarray']


def test_dryrun_lz4_scalar(stub_decoder, tmp_path):
    """LZ4 chunk: framing parse + python orchestration (kernel stubbed)."""
    from petastorm_amd.test_util.dataset_gen import create_scalar_dataset
    dec, stub = stub_decoder
    url = 'file://' + str(tmp_path / 'lz4ds')
    create_scalar_dataset(url, num_rows=2000, rowgroup_size=1000,
                          compression='lz4')
    out = _decode_all(dec, url, ['id', 'f0'])
    assert 'lz4_decompress_batch' in stub.calls
    assert stub.calls == _SEQ['lz4_scalar']
    assert not dec.cpu_assist_columns


def test_lz4_parse_framing_hadoop_and_raw():
    """Host-side framing detection: exact Hadoop framing is split into
    blocks; anything else is a single raw LZ4 block."""
    from petastorm_amd.gpu.decoder import GpuRowGroupDecoder
    blk1 = b'\x12' * 40          # opaque "compressed" payload
    blk2 = b'\x34' * 24
    framed = (len(blk1) + 4).to_bytes(4, 'big') + \
        len(blk1).to_bytes(4, 'big') + blk1 + \
        (60 - (len(blk1) + 4)).to_bytes(4, 'big') + \
        len(blk2).to_bytes(4, 'big') + blk2
    raw = b'\xAB' * 50
    buf = torch.from_numpy(
        np.frombuffer(framed + raw, dtype=np.uint8).copy())
    pages = {
        'data_off': torch.tensor([0, len(framed)], dtype=torch.int64),
        'comp_size': torch.tensor([len(framed), len(raw)],
                                  dtype=torch.int64),
        'uncomp_size': torch.tensor([60, 777], dtype=torch.int64),
    }
    b = GpuRowGroupDecoder._lz4_parse_framing(buf, pages)
    # page 0: two hadoop blocks; page 1: raw fallback
    np.testing.assert_array_equal(b['page'], [0, 0, 1])
    np.testing.assert_array_equal(b['src'], [8, 8 + len(blk1) + 8,
                                             len(framed)])
    np.testing.assert_array_equal(b['src_len'], [len(blk1), len(blk2), 50])
    np.testing.assert_array_equal(b['dst_rel'], [0, len(blk1) + 4, 0])
    np.testing.assert_array_equal(b['dst_len'], [len(blk1) + 4,
                                                 60 - (len(blk1) + 4), 777])


def test_zstd_host_decompress_matches_libzstd_oracle():
    """From-scratch RFC 8878 decoder vs data compressed by libzstd
    (ctypes oracle) across levels and data shapes."""
    import ctypes
    from petastorm_amd import ops
    ext = ops.ext()
    z = ctypes.CDLL('libzstd.so.1')
    z.ZSTD_compress.restype = ctypes.c_size_t
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    rng = np.random.RandomState(3)
    datas = [
        bytes(rng.randint(0, 256, 5000, dtype=np.uint8)),
        bytes(rng.randint(0, 7, 60000, dtype=np.uint8)),
        (b'abcdef' * 40000),                      # multi-block, matches
        rng.rand(20000).tobytes(),                # float pages
        b'x',
        bytes(200000),                            # zeros / RLE blocks
    ]
    comps = []
    for d, lvl in zip(datas, (1, 3, 9, 19, 1, 5)):
        buf = ctypes.create_string_buffer(z.ZSTD_compressBound(len(d)))
        n = z.ZSTD_compress(buf, len(buf.raw), d, len(d), lvl)
        comps.append(buf.raw[:n])
    blob = b''.join(comps)
    src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy())
    src_off, pos = [], 0
    for c in comps:
        src_off.append(pos)
        pos += len(c)
    src_len = [len(c) for c in comps]
    dst_len = [len(d) for d in datas]
    dst_off, pos = [], 0
    for n in dst_len:
        dst_off.append(pos)
        pos += n
    dst = torch.empty(pos, dtype=torch.uint8)
    status = torch.zeros(len(datas), dtype=torch.int32)
    ext.zstd_decompress_host(
        src, torch.tensor(src_off), torch.tensor(src_len),
        dst, torch.tensor(dst_off), torch.tensor(dst_len), status)
    assert status.tolist() == [0] * len(datas)
    out = dst.numpy().tobytes()
    for d, o, n in zip(datas, dst_off, dst_len):
        assert out[o:o + n] == d


def test_dryrun_zstd_scalar(stub_decoder, tmp_path):
    """ZSTD chunk: host decompression (real, native) + stubbed kernels."""
    from petastorm_amd.test_util.dataset_gen import create_scalar_dataset
    dec, stub = stub_decoder
    url = 'file://' + str(tmp_path / 'zstdds')
    create_scalar_dataset(url, num_rows=2000, rowgroup_size=1000,
                          compression='zstd')
    out = _decode_all(dec, url, ['id', 'f0'])
    assert not dec.cpu_assist_columns


def test_zstd_corrupt_page_raises(stub_decoder, tmp_path):
    """Bit-flipped ZSTD page payload must raise loudly (status contract),
    not return garbage."""
    import pyarrow.parquet as pq
    from petastorm_amd.test_util.dataset_gen import create_scalar_dataset
    dec, stub = stub_decoder
    url = 'file://' + str(tmp_path / 'zc')
    create_scalar_dataset(url, num_rows=2000, rowgroup_size=1000,
                          compression='zstd')
    path = [str(p) for p in (tmp_path / 'zc').iterdir()
            if p.suffix == '.parquet'][0]
    pf = pq.ParquetFile(path)
    col = pf.metadata.row_group(0).column(0)  # 'id': compressible int64
    # +200: clear of the thrift header (statistics make it ~100 bytes)
    off = col.data_page_offset + 200
    raw = bytearray(open(path, 'rb').read())
    for i in range(24):
        raw[off + i] ^= 0xA5
    open(path, 'wb').write(bytes(raw))
    with pytest.raises(RuntimeError, match='zstd'):
        _decode_all(dec, url, [col.path_in_schema])


@pytest.mark.parametrize('compression', ['snappy', 'none', 'gzip', 'zstd',
                                         'lz4'])
def test_dryrun_datapage_v2_paths(stub_decoder, tmp_path, compression):
    """DataPageV2 python orchestration for every codec (kernels stubbed;
    zstd host decompression is real)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from petastorm_amd.unischema import Unischema
    dec, stub = stub_decoder
    rng = np.random.RandomState(0)
    path = str(tmp_path / ('v2_' + compression + '.parquet'))
    pq.write_table(
        pa.table({'id': pa.array(np.arange(3000)),
                  'x': pa.array(rng.rand(3000))}),
        path, compression=compression, use_dictionary=False,
        row_group_size=1500, data_page_version='2.0')
    pf = pq.ParquetFile(path)
    schema = Unischema.from_arrow_schema(pf.schema_arrow)
    host, meta = dec.read_rowgroup_bytes(path, pf.metadata, pf.schema, 0,
                                         ['id', 'x'])
    out, _ = dec.decode(host, meta, schema)
    dec.flush_status()
    assert set(out) == {'id', 'x'}
    assert not dec.cpu_assist_columns


def test_dryrun_dictionary_paths(stub_decoder, tmp_path):
    """Dictionary-encoded chunk orchestration (kernels stubbed)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from petastorm_amd.unischema import Unischema
    dec, stub = stub_decoder
    vals = np.array([1.5, 2.5, 3.5])[np.random.RandomState(0)
                                     .randint(0, 3, 4000)]
    path = str(tmp_path / 'dict.parquet')
    # uncompressed: the dict path reads level-length prefixes from the
    # page bytes, which a stubbed decompression kernel cannot provide
    pq.write_table(pa.table({'x': pa.array(vals)}), path,
                   compression='none', use_dictionary=True,
                   row_group_size=2000)
    pf = pq.ParquetFile(path)
    schema = Unischema.from_arrow_schema(pf.schema_arrow)
    host, meta = dec.read_rowgroup_bytes(path, pf.metadata, pf.schema, 0,
                                         ['x'])
    out, _ = dec.decode(host, meta, schema)
    dec.flush_status()
    assert 'rle_hybrid_decode_batch' in stub.calls
    assert not dec.cpu_assist_columns
    assert stub.calls == _SEQ['dictionary']


def test_dryrun_npz_interop_column(stub_decoder, tmp_path):
    """Upstream-petastorm CompressedNdarrayCodec payloads are npz (zip)
    containers: the decoder must detect them and either decode through
    raw-DEFLATE segments or fall back — never feed zip bytes to the zlib
    path.  Kernels are stubbed, so this only proves the orchestration
    (zip probe, segment math, shapes) doesn't crash; value correctness is
    covered by the gpu-marked interop test."""
    from petastorm_amd.test_util.reference_store import \
        create_reference_style_dataset
    dec, stub = stub_decoder
    d = str(tmp_path / 'refz')
    create_reference_style_dataset(d, num_rows=8, rows_per_group=4)
    out, sch = _decode_all(dec, 'file://' + d, ['id', 'matrix_z'])
    z = dec.decode_compressed_ndarray_column(out['matrix_z'],
                                             sch.fields['matrix_z'])
    assert z is None or z.shape == (4, 4, 5)
    assert 'inflate_batch' in stub.calls or 'varlen_gather' in stub.calls
    assert stub.calls == _SEQ['npz']


def test_dryrun_string_column_host_visible_exact(stub_decoder, tmp_path):
    """Uncompressed REQUIRED string column: the device string path's
    host-visible branch materializes EXACT values with no GPU (and no
    pyarrow re-read) — value correctness of decode_string_column."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    dec, stub = stub_decoder
    d = tmp_path / 'strs'
    d.mkdir()
    vals = ['s-%d' % i for i in range(40)] + ['', 'unicode-é中']
    table = pa.Table.from_arrays(
        [pa.array(np.arange(len(vals), dtype=np.int64)),
         pa.array(vals, type=pa.string())],
        schema=pa.schema([pa.field('id', pa.int64(), nullable=False),
                          pa.field('name', pa.string(), nullable=False)]))
    pq.write_table(table, str(d / 'p.parquet'), compression='none',
                   use_dictionary=False)
    out, sch = _decode_all(dec, 'file://' + str(d), ['id', 'name'])
    col = out['name']
    assert isinstance(col, ByteArrayColumn) and col.host_buf is not None
    got = dec.decode_string_column(col, sch.fields['name'])
    assert got.tolist() == vals


def test_dryrun_list_column_takes_assist_not_crash(stub_decoder, tmp_path):
    """Repeated (list) columns must route to CPU assist gracefully — the
    leaf path ('col.list.element') used to KeyError in
    read_rowgroup_bytes."""
    from petastorm_amd.test_util.dataset_gen import create_rich_scalar_dataset
    dec, stub = stub_decoder
    d = str(tmp_path / 'rich')
    create_rich_scalar_dataset('file://' + d, num_rows=20, rowgroup_size=10)
    out, sch = _decode_all(dec, 'file://' + d,
                           ['id', 'int_fixed_size_list', 'string'])
    assert out['id'] is not None
    assert out['int_fixed_size_list'] is None  # assist marker
    assert 'int_fixed_size_list' in dec.cpu_assist_columns


def test_dryrun_delta_encodings(stub_decoder, tmp_path):
    """DELTA_BINARY_PACKED / DELTA_LENGTH_BYTE_ARRAY orchestration
    (kernels stubbed): shapes and kernel selection."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    dec, stub = stub_decoder
    d = tmp_path / 'delta'
    d.mkdir()
    n = 400
    table = pa.Table.from_arrays(
        [pa.array(np.arange(n, dtype=np.int64) * 3 - 100),
         pa.array(['v%d' % i for i in range(n)], pa.string())],
        schema=pa.schema([pa.field('i64', pa.int64(), nullable=False),
                          pa.field('s', pa.string(), nullable=False)]))
    pq.write_table(table, str(d / 'p.parquet'), row_group_size=200,
                   use_dictionary=False, compression='none',
                   column_encoding={'i64': 'DELTA_BINARY_PACKED',
                                    's': 'DELTA_LENGTH_BYTE_ARRAY'})
    out, sch = _decode_all(dec, 'file://' + str(d), ['i64', 's'])
    assert out['i64'] is not None and out['i64'].shape == (200,)
    assert out['s'] is not None and out['s'].n == 200
    assert 'delta_binary_packed_batch' in stub.calls
    assert 'delta_length_byte_array_batch' in stub.calls
    assert stub.calls == _SEQ['delta']
    assert not dec.cpu_assist_columns


def test_dryrun_bool_bss_delta_ba(stub_decoder, tmp_path):
    """BOOLEAN / BYTE_STREAM_SPLIT / DELTA_BYTE_ARRAY orchestration with
    stubbed kernels: kernel selection and shape plumbing."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    dec, stub = stub_decoder
    d = tmp_path / 'enc3'
    d.mkdir()
    n = 300
    table = pa.Table.from_arrays(
        [pa.array(np.random.rand(n).astype(np.float32)),
         pa.array(np.arange(n) % 2 == 0),
         pa.array(['p-%d' % (i // 5) for i in range(n)], pa.string())],
        schema=pa.schema([pa.field('f', pa.float32(), nullable=False),
                          pa.field('b', pa.bool_(), nullable=False),
                          pa.field('s', pa.string(), nullable=False)]))
    pq.write_table(table, str(d / 'p.parquet'), use_dictionary=False,
                   compression='none',
                   column_encoding={'f': 'BYTE_STREAM_SPLIT',
                                    's': 'DELTA_BYTE_ARRAY',
                                    'b': 'PLAIN'})
    out, sch = _decode_all(dec, 'file://' + str(d), ['f', 'b', 's'])
    assert out['f'] is not None and out['f'].shape == (n,)
    assert out['b'] is not None and out['b'].dtype == torch.bool
    assert out['s'] is not None and out['s'].n == n
    assert 'byte_stream_split_batch' in stub.calls
    assert 'bool_unpack_batch' in stub.calls
    assert 'delta_byte_array_lengths_batch' in stub.calls
    assert stub.calls == _SEQ['bool_bss_delta_ba']
    assert not dec.cpu_assist_columns


def test_dryrun_flba(stub_decoder, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    dec, stub = stub_decoder
    d = tmp_path / 'flba'
    d.mkdir()
    n = 100
    table = pa.Table.from_arrays(
        [pa.array(np.random.rand(n).astype(np.float16)),
         pa.array([b'ab12'] * n, pa.binary(4))],
        schema=pa.schema([pa.field('h', pa.float16(), nullable=False),
                          pa.field('fb', pa.binary(4), nullable=False)]))
    pq.write_table(table, str(d / 'p.parquet'), use_dictionary=False,
                   compression='none')
    out, sch = _decode_all(dec, 'file://' + str(d), ['h', 'fb'])
    assert out['h'] is not None and out['h'].dtype == torch.float16
    assert out['fb'] is not None and out['fb'].n == n
    # uncompressed fixed binary is host-visible: exact bytes on CPU
    got = dec.decode_string_column(out['fb'], sch.fields['fb'])
    assert got.tolist() == [b'ab12'] * n
    assert not dec.cpu_assist_columns


@pytest.mark.parametrize('compression', ['none', 'snappy', 'gzip', 'lz4',
                                         'zstd'])
@pytest.mark.parametrize('version', ['1.0', '2.0'])
def test_dryrun_nullable_pages_v1_v2(stub_decoder, tmp_path, version,
                                     compression):
    """Nullable PLAIN / DELTA_LENGTH_BYTE_ARRAY strings and nullable FLBA
    over several pages take the GPU route under every codec.  The expected
    launches do not depend on the page version: V1 and V2 give one and the
    same sequence."""
    from petastorm_amd.test_util.dataset_gen import \
        create_nullable_pages_dataset
    dec, stub = stub_decoder
    url = 'file://' + str(tmp_path / 'np')
    create_nullable_pages_dataset(url, version, compression)
    out, _ = _decode_all(dec, url, ['id', 's', 's2', 'fb'])
    assert not dec.cpu_assist_columns
    assert out['id'].shape == (600,)
    for name in ('s', 's2', 'fb'):
        assert isinstance(out[name], ByteArrayColumn)
        # the stubbed level decode yields all-zero levels: every row null
        assert out[name].n == 0 and out[name].valid.shape == (600,)
    # zstd decompresses on the host; the others once per column chunk
    decompress = {'snappy': 'snappy ', 'gzip': 'inflate_batch ',
                  'lz4': 'lz4 '}.get(compression, '')
    assert stub.calls == _seq(''.join(decompress + column for column in (
        'fixed ',                                  # id
        'rle ba_offsets ',                         # s
        'rle delta_length_byte_array_batch ',      # s2
        'rle ')))                                  # fb: offsets on the host


def test_cuda_route_requires_gpu_at_construction(tmp_path):
    """device='cuda' on a GPU-less machine fails at CONSTRUCTION with a
    clear message, not at first batch."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('machine has a GPU')
    from petastorm_amd import make_batch_reader
    from petastorm_amd.test_util.dataset_gen import create_scalar_dataset
    url = 'file://' + str(tmp_path / 'sc')
    create_scalar_dataset(url, num_rows=50, rowgroup_size=25)
    with pytest.raises(RuntimeError, match='requires a GPU'):
        make_batch_reader(url, device='cuda')
