"""CPU: what `bench.py --full` switches.  A plain run measures the headline figure alone; the legs that take runs of
their own (cpu_baseline with its oracle comparison, the c5 and .npy also-runs) belong to --full."""
import pytest

import bench


def parse(monkeypatch, *argv):
    monkeypatch.setattr('sys.argv', ['bench.py'] + list(argv))
    return bench.parse()


@pytest.mark.parametrize('argv', [(), ('--gpus', '1', '--steps', '3', '--warmup', '2'), ('--workload', 'c5'),
                                  ('--cpu-sample', '4096', '--also', '1'), ('--dump-outputs', 'd')])
def test_plain_run_has_no_extra_legs(monkeypatch, argv):
    a = parse(monkeypatch, *argv)
    assert not a.full and a.also == 0 and a.cpu_sample == 0


def test_full_run_keeps_the_legs_and_their_switches(monkeypatch):
    a = parse(monkeypatch, '--full')
    assert a.full and a.also == 1 and a.cpu_sample == 14336
    a = parse(monkeypatch, '--full', '--also', '0', '--cpu-sample', '4096')
    assert a.full and a.also == 0 and a.cpu_sample == 4096


def test_full_leaves_the_timed_run_alone(monkeypatch):
    """--full adds legs after the timed steps: nothing that shapes the steps or their inputs depends on it."""
    plain = vars(parse(monkeypatch, '--steps', '5', '--warmup', '2'))
    full = vars(parse(monkeypatch, '--steps', '5', '--warmup', '2', '--full'))
    for k in ('full', 'also', 'cpu_sample'):
        plain.pop(k), full.pop(k)
    assert plain == full


def test_extra_legs_are_entered_only_by_their_switches(monkeypatch):
    """The segmentation body reaches cpu_baseline through args.cpu_sample and main() reaches also_runs through
    args.also: with both at 0 neither is called (the GPU body stubbed out, the legs made to fail if entered)."""
    called = []
    monkeypatch.setattr(bench, 'bench_segmentation', lambda a: called.append(a.cpu_sample) or {"metric": "m"})
    monkeypatch.setattr(bench, 'also_runs', lambda a: called.append('also') or {})
    monkeypatch.delenv('RANK', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('SHEPSEG_FORCE_DIST', raising=False)
    monkeypatch.setenv('SHEPSEG_DEVICE', '0')          # main() would set it for the process otherwise
    monkeypatch.setattr('sys.argv', ['bench.py'])
    bench.main()
    assert called == [0]
    del called[:]
    monkeypatch.setattr('sys.argv', ['bench.py', '--full'])
    bench.main()
    assert called == [14336, 'also']
