"""Benchmark harness, ReaderMock and CLI tools (parity: reference
tests/test_benchmark.py + tool smoke coverage)."""
import numpy as np
import pytest

from petastorm_amd.benchmark.dummy_reader import DummyReader
from petastorm_amd.benchmark.throughput import reader_throughput
from petastorm_amd.pytorch import BatchedDataLoader
from petastorm_amd.test_util.dataset_gen import TestSchema
from petastorm_amd.test_util.reader_mock import ReaderMock


def test_reader_throughput_on_dataset(test_dataset):
    result = reader_throughput(test_dataset['url'], warmup_cycles_count=5,
                               measure_cycles_count=20, loaders_count=2)
    assert result.samples_per_second > 0
    assert result.time_mean > 0


def test_reader_throughput_batch_method(test_dataset):
    result = reader_throughput(test_dataset['url'], warmup_cycles_count=1,
                               measure_cycles_count=2, loaders_count=2,
                               read_method='batch')
    assert result.samples_per_second > 0


def test_benchmark_cli(test_dataset, capsys):
    from petastorm_amd.benchmark.cli import main
    rc = main([test_dataset['url'], '-w', '2', '-m', '10', '-l', '2'])
    assert rc == 0
    assert 'samples/sec' in capsys.readouterr().out


def test_dummy_reader_with_loader():
    reader = DummyReader()
    loader = BatchedDataLoader(reader, batch_size=256)
    it = iter(loader)
    batch = next(it)
    assert batch['value'].shape == (256, 64)


def test_reader_mock():
    mock = ReaderMock(TestSchema)
    row = next(mock)
    assert row.matrix.shape == (10, 20)
    assert isinstance(row.id, np.int64)


def test_copy_dataset(test_dataset, tmp_path):
    from petastorm_amd import make_reader
    from petastorm_amd.tools.copy_dataset import copy_dataset
    target = 'file://' + str(tmp_path / 'copy')
    n = copy_dataset(test_dataset['url'], target,
                     field_regex=['id', 'matrix', 'matrix_nullable'],
                     not_null_fields=['matrix_nullable'])
    expected = [r for r in test_dataset['rows']
                if r['matrix_nullable'] is not None]
    assert n == len(expected)
    with make_reader(target, reader_pool_type='dummy',
                     shuffle_row_groups=False) as r:
        rows = list(r)
    assert len(rows) == len(expected)
    assert set(rows[0]._fields) == {'id', 'matrix', 'matrix_nullable'}


def test_generate_metadata_roundtrip(scalar_dataset):
    from petastorm_amd.etl.petastorm_generate_metadata import generate_metadata
    schema = generate_metadata(scalar_dataset['url'])
    # store is now readable via make_reader (schema was inferred + persisted)
    from petastorm_amd import make_reader
    with make_reader(scalar_dataset['url'], reader_pool_type='dummy',
                     shuffle_row_groups=False,
                     schema_fields=['id', 'f0']) as r:
        rows = list(r)
    assert len(rows) == 500


def test_metadata_util_cli(test_dataset, capsys):
    from petastorm_amd.etl.metadata_util import main
    rc = main([test_dataset['url'], '--print-schema', '--print-row-groups'])
    assert rc == 0
    out = capsys.readouterr().out
    assert 'row groups' in out and 'image_png' in out


def test_shuffling_analysis(tmp_path):
    from petastorm_amd.test_util.shuffling_analysis import (
        compute_correlation_distribution, generate_shuffle_analysis_dataset)
    url = 'file://' + str(tmp_path / 'shuffle_ds')
    generate_shuffle_analysis_dataset(url, num_rows=400, row_group_size=40)
    mean1, std1 = compute_correlation_distribution(
        url, 'id', shuffle_row_drop_partitions=1, num_corr_samples=5)
    mean2, std2 = compute_correlation_distribution(
        url, 'id', shuffle_row_drop_partitions=2, num_corr_samples=5)
    # shuffled orders decorrelate from the natural order (unseeded
    # statistic: generous bound keeps the assertion meaningful without
    # rare-tail flakes; with 10 row groups E[|corr|] is ~0.2)
    assert mean1 < 0.7 and mean2 < 0.7
    assert std1 >= 0.0 and std2 >= 0.0


def test_reader_throughput_spawned_process(test_dataset):
    """reference throughput.py:144-149 self-respawn for clean RSS"""
    result = reader_throughput(test_dataset['url'], warmup_cycles_count=2,
                               measure_cycles_count=5, loaders_count=2,
                               spawn_new_process=True)
    assert result.samples_per_second > 0


def test_bench_py_contract(tmp_path):
    """bench.py (driver contract): helloworld config on CPU prints one JSON
    line with the required keys, and the timed region respects
    --min-region."""
    import json
    import os
    import subprocess
    import sys
    env = dict(os.environ, PSA_BENCH_DATA=str(tmp_path))
    out = subprocess.run(
        [sys.executable, 'bench.py', '--config', 'helloworld',
         '--steps', '3', '--warmup', '1', '--batch-size', '10',
         '--min-region', '1.0'],
        capture_output=True, text=True, timeout=300,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith('{')][-1]
    j = json.loads(line)
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup',
                'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
                'dtype', 'data', 'config'):
        assert key in j, key
    assert j['steps'] == 3 and j['n_gpus'] == 1
    # loose bound: CPU-contended CI runs overestimate per-batch cost at
    # calibration, then run the timed region faster
    assert j['timed_region_s'] >= 0.2
    assert j['config']['batches_per_step'] >= 1


def _run_bench(tmp_path, argv):
    """Run bench.py in a fresh process; returns its JSON result line."""
    import json
    import os
    import subprocess
    import sys
    import time
    env = dict(os.environ, PSA_BENCH_DATA=str(tmp_path / 'data'))
    t0 = time.perf_counter()
    out = subprocess.run(
        [sys.executable, 'bench.py'] + argv,
        capture_output=True, text=True, timeout=300,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        env=env)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    j = json.loads(lines[0])
    # warmup and timed steps are the same size: all of them together fit
    # in the run
    assert 0 < (j['steps'] + j['warmup']) * j['ms_per_step'] / 1e3 <= wall
    return j, out.stderr


def _load_dump(d):
    import os
    return {f: np.load(os.path.join(str(d), f)) for f in sorted(os.listdir(str(d)))}


def _assert_dumps_equal(tmp_path, argv, extra_a=()):
    """Two fresh runs with the same arguments dump the same arrays
    (``extra_a``: options for the first run that must not change them).
    Returns the first run's result line, the arrays and both stderrs."""
    j1, err1 = _run_bench(tmp_path, argv + list(extra_a) +
                          ['--dump-outputs', str(tmp_path / 'a')])
    j2, err2 = _run_bench(tmp_path,
                          argv + ['--dump-outputs', str(tmp_path / 'b')])
    a, b = _load_dump(tmp_path / 'a'), _load_dump(tmp_path / 'b')
    assert a and sorted(a) == sorted(b)
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    for name in a:
        assert name.endswith('.npy')
        assert a[name].dtype in (np.float32, np.float64), name
        assert a[name].size > 0, name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    for j in (j1, j2):
        # a dump run takes one loader batch per step, whatever --min-region,
        # and its result line says so
        assert j['config']['batches_per_step'] == 1
        assert j['config']['min_region_s'] == 0
        assert j['ms_per_step'] > 0
    return j1, a, err1, err2


def test_bench_py_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed batch as float .npy files,
    identically from run to run; --full is accepted and leaves the result
    line's keys and fixed fields as they are (this config has no stage
    diagnostics to add; the GPU test below checks those)."""
    argv = ['--config', 'helloworld', '--rows', '40', '--steps', '2',
            '--warmup', '1', '--batch-size', '5']
    j, dump, _, _ = _assert_dumps_equal(tmp_path, argv)
    assert j['steps'] == 2 and j['warmup'] == 1
    assert {'id.npy', 'image1.npy', 'array_4d.npy'} <= set(dump)
    assert dump['image1.npy'].shape == (128, 256, 3)

    plain, _ = _run_bench(tmp_path, argv + ['--min-region', '0.2'])
    full, _ = _run_bench(tmp_path, argv + ['--min-region', '0.2', '--full'])
    assert sorted(plain) == sorted(full)
    for key in ('metric', 'unit', 'higher_is_better', 'dtype', 'steps'):
        assert plain[key] == full[key], key
    # a calibrated run is told apart from a dump run by its result line
    assert plain['config']['min_region_s'] == 0.2
    assert plain['config']['prime_batches'] == 1


def test_bench_py_warmup_steps_match_timed_steps(tmp_path):
    """With a calibrated region (several loader batches per step) and more
    warmup than timed steps, (steps + warmup) * ms_per_step still fits in
    the run's wall time (checked in _run_bench)."""
    j, _ = _run_bench(tmp_path, ['--config', 'helloworld', '--rows', '40',
                                 '--steps', '2', '--warmup', '4',
                                 '--batch-size', '5', '--min-region', '0.5'])
    assert j['steps'] == 2 and j['warmup'] == 4
    assert j['config']['batches_per_step'] > 1


def _stability_probe():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        'stability_probe', os.path.join(root, 'tools', 'stability_probe.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stability_probe_namespace_drives_bench(tmp_path, monkeypatch):
    """tools/stability_probe.py drives the bench_* functions with its own
    hand-built namespace and its own timing loop (old five-argument
    signature): step() and the code after the loop must work with both."""
    import torch
    import bench
    probe = _stability_probe()
    monkeypatch.setenv('PSA_BENCH_DATA', str(tmp_path))
    args = probe.bench_args('helloworld')
    assert not hasattr(args, 'dump_outputs') and not hasattr(args, 'full')
    args.rows, args.batch_size = 40, 5
    got = []

    def fake_run_timed(a, step_fn, dev, dist, world):
        got.extend([step_fn(), step_fn()])
        return {'elapsed_s': 1.0, 'samples': sum(got), 'ms_per_step': 500.0}

    monkeypatch.setattr(bench, '_run_timed', fake_run_timed)
    result, _ = bench.bench_helloworld_cpu(args, 0, 1, torch.device('cpu'),
                                           None)
    assert got == [5, 5] and result['samples'] == 10
    assert bench._timing_wanted(args) is False


@pytest.mark.gpu
def test_stability_probe_runs_flagship_config(tmp_path, monkeypatch):
    """The probe's own run_config() on the imagenet pipeline (small store,
    half a second): every step and the teardown run with its namespace."""
    import sys
    probe = _stability_probe()
    monkeypatch.setenv('PSA_BENCH_DATA', str(tmp_path))
    monkeypatch.setenv('PSA_IMAGENET_RPG', '32')   # 24 x 32 = 768 rows
    monkeypatch.delenv('PSA_SCALAR_COMPRESSION', raising=False)
    monkeypatch.delenv('PSA_TIMING', raising=False)
    monkeypatch.setattr(sys, 'argv', list(sys.argv))
    monkeypatch.setattr(sys, 'path', list(sys.path))
    windows = probe.run_config('imagenet', 0.5)
    assert windows == []   # a window is 5 s long; none closes in 0.5 s


@pytest.mark.gpu
def test_bench_py_dump_outputs_gpu(tmp_path, monkeypatch):
    """Flagship config: the dumped last batch (normalized NCHW fp32 images +
    labels) is identical across two fresh runs, with or without --full;
    --full adds the stage diagnostics on stderr, a run without it has
    none."""
    monkeypatch.setenv('PSA_IMAGENET_RPG', '64')
    monkeypatch.delenv('PSA_TIMING', raising=False)
    argv = ['--gpus', '1', '--rows', '256', '--batch-size', '32',
            '--steps', '3', '--warmup', '2']
    j, dump, err_full, err_plain = _assert_dumps_equal(
        tmp_path, argv, extra_a=['--full'])
    assert 'stage_times:' in err_full and 'staging_allocs:' in err_full
    assert 'stage_times:' not in err_plain
    assert j['dtype'] == 'fp32' and j['steps'] == 3
    assert dump['image.npy'].shape == (32, 3, 224, 224)
    assert dump['image.npy'].dtype == np.float32
    assert dump['label.npy'].shape == (32,)
    # labels are row index % 1000 of a 256-row store
    lab = dump['label.npy']
    assert np.all(lab == np.round(lab)) and lab.min() >= 0 and lab.max() < 256
    assert np.isfinite(dump['image.npy']).all()


def test_reencode_dataset_adds_restart_markers(tmp_path):
    """Foreign-style (no-RST) jpeg dataset re-encoded for parallel GPU
    Huffman decode: output carries DRI/RSTn markers and images stay
    visually identical (one jpeg generation loss)."""
    import os
    import numpy as np
    from petastorm_amd import make_reader
    from petastorm_amd.test_util.dataset_gen import create_imagenet_dataset
    from petastorm_amd.tools.reencode_dataset import reencode_dataset

    src = 'file://' + str(tmp_path / 'src')
    dst = 'file://' + str(tmp_path / 'dst')
    os.environ['PSA_JPEG_RST_BLOCKS'] = '0'  # foreign-style: no markers
    try:
        create_imagenet_dataset(src, num_rows=6, rowgroup_size_mb=8)
    finally:
        del os.environ['PSA_JPEG_RST_BLOCKS']

    rows, cols = reencode_dataset(src, dst, rst_blocks=2, quality=95)
    assert rows == 6 and cols == ['image']

    import pyarrow.parquet as pq
    import glob
    src_file = glob.glob(str(tmp_path / 'src' / '*.parquet'))[0]
    dst_file = glob.glob(str(tmp_path / 'dst' / '*.parquet'))[0]
    src_jpg = pq.read_table(src_file, columns=['image'])['image'][0].as_py()
    dst_jpg = pq.read_table(dst_file, columns=['image'])['image'][0].as_py()
    assert b'\xff\xdd' not in src_jpg      # no DRI in foreign source
    assert b'\xff\xdd' in dst_jpg          # DRI present after re-encode
    assert any(bytes([0xFF, 0xD0 + i]) in dst_jpg for i in range(8))

    with make_reader(src, reader_pool_type='dummy',
                     shuffle_row_groups=False) as r1, \
            make_reader(dst, reader_pool_type='dummy',
                        shuffle_row_groups=False) as r2:
        for a, b in zip(r1, r2):
            assert a.label == b.label
            diff = np.abs(a.image.astype(np.int16) -
                          b.image.astype(np.int16))
            assert diff.mean() < 6  # one extra jpeg generation at q95


def test_examples_run(tmp_path):
    """The example scripts execute end to end on CPU (reference keeps
    per-example tests, examples/*/tests)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for script, args in (
            ('examples/hello_world/main.py',
             ['file://' + str(tmp_path / 'hw_ex')]),
            ('examples/hello_world/external_dataset.py', []),
            ('examples/mnist/main.py', []),
            ('examples/spark_converter/main.py', ['--rows', '96']),
    ):
        out = subprocess.run([sys.executable, os.path.join(root, script)]
                             + args, capture_output=True, text=True,
                             timeout=240, cwd=root)
        assert out.returncode == 0, (script, out.stderr[-1500:])
