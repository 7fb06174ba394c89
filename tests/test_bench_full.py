"""`bench.py` plain and `--full`: a plain run carries the headline alone; every leg measured outside the timed steps sits behind `--full`."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT

HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'n_gpus')
LEGS = ('other_mode', 'f16_mode', 'geometry', 'config3', 'config5', 'cpu_baseline', 'logit_max_abs_err_vs_oracle', 'mask_disagree_vs_oracle')


def test_legs_are_off_in_a_plain_run_and_on_under_full():
    import bench
    legs = lambda a: (not a.no_other_modes, not a.no_extra_legs, not a.no_cpu_baseline)
    plain = bench.parse_args(['--gpus', '1', '--steps', '20', '--warmup', '5'])
    assert not plain.full and legs(plain) == (False, False, False)
    assert legs(bench.parse_args(['--no-cpu-baseline', '--dump-outputs', 'd'])) == (False, False, False)
    assert legs(bench.parse_args(['--full'])) == (True, True, True)
    assert legs(bench.parse_args(['--full', '--no-cpu-baseline'])) == (True, True, False)
    assert legs(bench.parse_args(['--full', '--no-extra-legs'])) == (True, False, True)
    timed = lambda a: (a.gpus, a.steps, a.warmup, a.batch, a.precision, a.workload, a.no_profile)
    full = bench.parse_args(['--gpus', '1', '--steps', '20', '--warmup', '5', '--full'])
    assert timed(full) == timed(plain) == (1, 20, 5, 64, 'split', 'config2', False)       # the option leaves what is timed alone


def _line(*argv, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', *argv],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE) and out['steps'] == 3 and out['warmup'] == 1 and out['value'] > 0
    assert out['metric'] == '2-ch 512x512 slices/sec' and out['unit'] == 'slices/s' and out['higher_is_better'] is True
    assert abs(out['value'] - 64 * 1e3 / out['ms_per_step']) <= 1e-3 * out['value']
    assert out['profiled_steps'] == 1 and out['roofline']['frac'] > 0          # the events sampled inside the timed steps: every line
    return out


@pytest.mark.gpu
def test_plain_line_is_the_headline_without_any_leg():
    out = _line(timeout=300)
    assert not [k for k in LEGS if k in out]


@pytest.mark.gpu
def test_full_line_carries_every_leg():
    out = _line('--full', timeout=600)
    assert not [k for k in LEGS if k not in out]
    assert out['other_mode']['precision_mode'] == 'exact' and out['other_mode']['value'] > 0 and out['f16_mode']['value'] > 0
    for leg in ('geometry', 'config3', 'config5'):
        assert 'error' not in out[leg], out[leg]
    assert set(out['geometry']) >= {'512x512', '640x384', '448x576_7stages'} and out['config3']['labels'] == 117
    assert out['cpu_baseline']['value'] > 0
    err = out['logit_max_abs_err_vs_oracle']
    assert err['value'] <= err['tol'] and out['mask_disagree_vs_oracle']['flips_all_within_logit_error_of_threshold']
