"""TEST INFRASTRUCTURE (never imported by the product): builds tests/plan_driver.cpp - the host planners csrc/dispatch.cpp, csrc/program.cpp and
csrc/tiled_plan.cpp behind a main of their own - under the address and undefined-behaviour sanitizers, and spells a network for it.  The
program has its own ``main``, touches no device and is never loaded into Python; it runs with leak checking on."""
import os
import shutil
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
MODE_ID = {'exact': 0, 'split': 1, 'f16': 2}          # TS2D_PRECISION_* of include/ts2d_engine.h
TIMES = {}                                            # 'compile' / the runs: seconds, printed by the tests (pytest -s)
_BUILT = []                                           # the program of this session: both modules run the same one


def build(tmp_dir):
    """The Makefile's host line (hipcc -x c++ -D__HIP_PLATFORM_AMD__ -I$(HIP_INC)) plus -O1 -g and the two sanitizers."""
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc: the planners include the HIP runtime API header')
    if _BUILT and os.path.exists(_BUILT[0]):
        return _BUILT[0]
    exe = os.path.join(str(tmp_dir), 'plan_driver')
    inc = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), 'include')
    t0 = time.time()
    subprocess.check_call([HIPCC, '-x', 'c++', '-D__HIP_PLATFORM_AMD__', '-I' + inc, '-I' + CSRC, '-O1', '-g', '-std=c++17', '-Wall', '-Wno-unused-function',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe, os.path.join(ROOT, 'tests', 'plan_driver.cpp'),
                           os.path.join(CSRC, 'dispatch.cpp'), os.path.join(CSRC, 'program.cpp'), os.path.join(CSRC, 'tiled_plan.cpp')])
    TIMES['compile'] = time.time() - t0
    _BUILT[:] = [exe]
    return exe


def run(exe, args, what):
    """stdout lines of a run that ended clean: status 0 and nothing from a sanitizer (leaks included) on stderr."""
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1', UBSAN_OPTIONS='print_stacktrace=1')
    t0 = time.time()
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env)
    TIMES[what] = time.time() - t0
    assert res.returncode == 0 and not res.stderr.strip(), (what, res.returncode, res.stderr[-4000:])
    return res.stdout.split('\n')[:-1]


def net_words(name, arch):
    """The `net` line of a sweep: the fields engine._desc / engine._residual_desc copy into the C descriptors."""
    arch.validate()
    residual = arch.encoder == 'residual'
    n = arch.n_stages
    w = ['net', name, int(residual), arch.input_channels, arch.num_classes, n]
    w += [int(f) for f in arch.features_per_stage]
    w += [int(c) for c in arch.n_conv_per_stage]
    w += [int(c) for c in arch.n_conv_per_stage_decoder]
    for st in arch.strides:
        w += [int(st[0]), int(st[1])]
    if residual:
        w += [int(b) for b in arch.n_blocks_per_stage]
    return ' '.join(str(v) for v in w)
