"""bench.py's --gpus N contract on the CPU (no GPU calls): N > 1 outside a launcher starts N ranks
through torch.distributed.run as a child process, a node with fewer GPUs fails loudly, and a rank
whose launcher started a different world size than --gpus refuses to run (it would otherwise print an
`n_gpus` that is not what was asked for)."""
import json
import os
import subprocess
import sys
import types

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), *args], env=env, capture_output=True,
                          text=True, timeout=300)


def test_gpus_more_than_present_fails():
    # more GPUs than any node has: fails before launching ranks, whatever machine runs the test
    r = _run(['--gpus', '4096'])
    assert r.returncode != 0
    assert 'needs 4096 GPUs' in r.stderr
    assert '"n_gpus"' not in r.stdout


def test_world_mismatch_fails():
    r = _run(['--gpus', '4'], {'WORLD_SIZE': '2', 'RANK': '0', 'LOCAL_RANK': '0'})
    assert r.returncode == 2
    assert 'launcher started 2 rank(s)' in r.stderr


def test_launcher_command(monkeypatch):
    import bench
    seen = {}
    monkeypatch.setattr(bench.torch.cuda, 'device_count', lambda: 8)

    def fake_run(cmd, env=None):
        seen['cmd'], seen['env'] = cmd, env
        return types.SimpleNamespace(returncode=7)
    monkeypatch.setattr(subprocess, 'run', fake_run)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--steps', '3'])
    args = types.SimpleNamespace(gpus=4)
    assert bench.launch_ranks(args) == 7
    cmd = seen['cmd']
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert '--nproc-per-node=4' in cmd and '--nnodes=1' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert cmd[-4:] == ['--gpus', '4', '--steps', '3'] and cmd[-5].endswith('bench.py')
    assert seen['env']['PNR_DIST_BACKEND'] == 'nccl'


def test_main_launches_when_no_world(monkeypatch):
    import bench
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '2'])
    monkeypatch.setattr(bench, 'launch_ranks', lambda a: 0 if a.gpus == 2 else 1)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0


def _stub_two_ranks(monkeypatch, argv):
    """Rank 0 of a 2-rank bench.main() with every GPU workload stubbed (no GPU, no process group);
    returns the list the stubs append their calls to."""
    import bench
    from pnr import dist as pdist
    import pnr
    calls = []
    monkeypatch.setenv('WORLD_SIZE', '2')
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
    monkeypatch.setattr(bench.torch.cuda, 'device_count', lambda: 2)
    monkeypatch.setattr(bench.torch.cuda, 'set_device', lambda d: None)
    monkeypatch.setattr(pdist, 'init', lambda backend=None: (0, 2, 0))

    class DP:
        world = 2

        def barrier(self):
            calls.append('barrier')
    monkeypatch.setattr(pdist, 'DataParallel', DP)
    import torch.distributed as tdist
    monkeypatch.setattr(tdist, 'get_backend', lambda *a: 'nccl')
    monkeypatch.setattr(tdist, 'get_world_size', lambda *a: 2)
    monkeypatch.setattr(tdist, 'destroy_process_group', lambda *a: calls.append('destroy'))
    monkeypatch.setattr(pnr, 'library', lambda: None)
    monkeypatch.setattr(bench, 'load_scene', lambda: (None, None, {'w': 0}))

    def room0(*a, **k):
        calls.append(('room0', k.get('steps'), k.get('warmup'), k.get('full'), k.get('dump')))
        return {'rays_per_s': 1.0e6, 'ms_per_iter': 1.0, 'workload': 'room0', 'rays_per_iter': 1000,
                'roofline': {'frac': 0.3}, 'cpu_baseline': None}
    monkeypatch.setattr(bench, 'room0_extra', room0)

    def smap(*a, **k):
        calls.append('smap')
        return {'value': 5.0e6, 'n_gpus': a[-2] if len(a) > 11 else 2}
    monkeypatch.setattr(bench, 'smap_run', smap)

    def fixed_global(*a, **k):
        calls.append('fixed_global')
        return {'value': 4.0e6, 'scaling': 'strong'}
    monkeypatch.setattr(bench, 'fixed_global_run', fixed_global)

    def sfwd(*a, **k):
        calls.append(('sfwd', k.get('world'), k.get('fixed_global', False)))
        return {'value': 2.0e7, 'n_gpus': k.get('world'), 'scaling': 'strong' if k.get('fixed_global') else 'weak'}
    monkeypatch.setattr(bench, 'sfwd_extra', sfwd)

    def gather(dev, feat_dtype='float32'):
        calls.append('gather')
        return {'frac': 0.5}
    monkeypatch.setattr(bench, 'gather_roofline', gather)
    return calls


def test_rank0_line_at_n2_carries_the_scaling_keys(monkeypatch, capsys):
    """Rank 0's line of a 2-rank `--full` run (every GPU workload stubbed: no GPU, no process group)
    carries the keys the driver's 1/2/4/8 curve reads -- the headline, `smap`, `fixed_global_batch`, the
    north star's S-fwd batch in its weak and fixed-global forms, the gather line and `distributed` --
    with the same key names as the N = 1 line."""
    import bench
    calls = _stub_two_ranks(monkeypatch, ['--gpus', '2', '--steps', '3', '--warmup', '1', '--full'])
    bench.main()
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out['n_gpus'] == 2 and out['value'] == 2.0e6
    assert out['distributed']['world_size'] == 2
    for key in ('smap', 'smap_value', 'fixed_global_batch', 'sfwd', 'sfwd_fixed_global', 'gather_roofline'):
        assert key in out, key
    assert out['sfwd']['scaling'] == 'weak' and out['sfwd_fixed_global']['scaling'] == 'strong'
    assert ('sfwd', 2, False) in calls and ('sfwd', 2, True) in calls
    assert calls[-2:] == ['barrier', 'destroy']


def test_plain_run_measures_the_headline_only(monkeypatch, capsys, tmp_path):
    """Without --full the run times its own steps and nothing else: no extra workload, CPU leg or
    gather line is started, --steps / --warmup / --dump-outputs reach the timed workload, and the
    line still holds the headline keys."""
    import bench
    dump = str(tmp_path / 'out')
    calls = _stub_two_ranks(monkeypatch, ['--gpus', '2', '--steps', '7', '--warmup', '2', '--dump-outputs', dump])
    bench.main()
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert calls == [('room0', 7, 2, False, dump), 'barrier', 'destroy']
    assert out['steps'] == 7 and out['warmup'] == 2 and out['ms_per_step'] == 1.0
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in out, key
    for key in ('smap', 'smap_value', 'fixed_global_batch', 'sfwd', 'sfwd_fixed_global', 'gather_roofline'):
        assert key not in out, key


def test_dump_outputs_writes_float32_arrays(tmp_path):
    """--dump-outputs' writer: one float32 .npy per name (a 0-d loss as one element), and an array
    above the per-array cap stored as the same seeded sample of its elements on every call."""
    import numpy as np
    import torch
    import bench
    big = torch.arange(bench.DUMP_MAX_ELEMS + 5, dtype=torch.float64)
    arrays = {'loss': torch.tensor(2.5), 'grid': torch.ones(3, 4, dtype=torch.float64), 'big': big}
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    bench.dump_outputs(a, arrays)
    bench.dump_outputs(b, arrays)
    loss, grid, s = (np.load(os.path.join(a, n + '.npy')) for n in ('loss', 'grid', 'big'))
    assert loss.dtype == np.float32 and loss.shape == (1,) and loss[0] == 2.5
    assert grid.dtype == np.float32 and grid.shape == (3, 4)
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_MAX_ELEMS,) and (np.diff(s) > 0).all()
    assert np.array_equal(s, np.load(os.path.join(b, 'big.npy')))
    assert sorted(os.listdir(a)) == ['big.npy', 'grid.npy', 'loss.npy']
