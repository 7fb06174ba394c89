"""Build-time checks of the emitted stream of conv3x3s2_v2p (csrc/kernels_s2v2p.h), without a GPU.

The kernel takes its B operand from L2 through a register ring two taps deep and waits for it with the vmcnt(N) that hipcc counts - nothing
is hand-counted - but its speed rests on three properties that a compiler upgrade or a careless edit can silently undo:
  * no register spills: at ~255 of 256 VGPRs a scratch reload would sit between the MFMAs, and it retires the whole vmcnt queue;
  * no `s_waitcnt vmcnt(0)` between the MFMAs of the item loop: vmcnt retires in order, so such a wait drains the patch requests of the item
    after next and the ring at once;
  * the wait in front of a tap's first MFMA leaves the loads issued BEHIND the awaited ring fragment in flight: N equals the number of
    vector-memory operations between that fragment's load and the wait (straight-line taps; the taps whose load lies in the previous item are
    reached over several paths and only bounded from below).
As tests/test_kernel_isa.py does, engine.hip is compiled to assembly here with the device flags of the shipped build (`make flags`; hipcc
cross-compiles without a GPU)."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

HIPCC = '/opt/rocm/bin/hipcc'
CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')


@pytest.fixture(scope='module')
def body(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    out = tmp_path_factory.mktemp('s2p_isa') / 'engine.s'
    src = os.path.join(CSRC, 'engine.hip')
    devflags = subprocess.check_output(['make', '-s', '-C', CSRC, 'flags'], text=True).split()
    subprocess.check_call([HIPCC, '-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-S', *devflags, '-o', str(out), src],
                          stderr=subprocess.DEVNULL)
    asm = open(out).read()
    m = re.search(r'^(_ZN4ts2d\w*conv3x3s2_v2p\w*):', asm, re.M)
    assert m, 'conv3x3s2_v2p not found in the assembly'
    text = asm[asm.index('\n', m.end()):asm.index('.Lfunc_end', m.end())]
    lines = [ln.split(';')[0].strip() for ln in text.split('\n')]           # (comments dropped: a loop header's label carries one)
    return [ln for ln in lines if ln]


def _is_vmem(ln):
    return ln.split()[0].startswith(('buffer_', 'global_', 'scratch_', 'flat_'))


def _loop(body):
    """[first, last] line of the item loop: from the label the loop's backward branch names to that branch."""
    labels = {ln[:-1]: i for i, ln in enumerate(body) if ln.endswith(':')}
    back = [(labels[ln.split()[-1]], i) for i, ln in enumerate(body)
            if ln.startswith(('s_cbranch', 's_branch')) and ln.split()[-1] in labels and labels[ln.split()[-1]] < i
            and sum('v_mfma' in x for x in body[labels[ln.split()[-1]]:i]) >= 2 * 108]
    assert back, 'no backward branch around two items of 108 MFMAs'
    return max(back, key=lambda b: b[1] - b[0])


def test_no_spills(body):
    assert not [ln for ln in body if ln.startswith('scratch_')], 'conv3x3s2_v2p spills registers'


def test_no_full_drain_between_the_mfmas(body):
    lo, hi = _loop(body)
    mf = [i for i in range(lo, hi) if 'v_mfma' in body[i]]
    assert len(mf) == 2 * 108, len(mf)                       # two items x 9 taps x 12 products
    bad = [i for i in range(mf[0], mf[-1]) if body[i].startswith('s_waitcnt') and 'vmcnt(0)' in body[i]]
    assert not bad, [body[i] for i in bad]


def test_ring_waits_match_the_issue_order(body):
    lo, hi = _loop(body)
    exact = bounded = 0
    for i in range(lo, hi):
        m = re.match(r's_waitcnt vmcnt\((\d+)\)', body[i])
        if not m or 'v_mfma' not in body[i + 1]:
            continue
        n = int(m.group(1))
        breg = body[i + 1].split(',')[2].strip()             # B operand of the MFMA behind the wait: a ring fragment
        younger, j, straight = 0, i - 1, True
        while j >= lo and not (body[j].startswith('buffer_load_dwordx4 ' + breg + ',')):
            younger += _is_vmem(body[j])
            straight &= not body[j].endswith(':')
            j -= 1
        if j < lo:                                           # loaded by the previous item: several paths lead here
            assert n >= 5, (body[i], body[i + 1])
            bounded += 1
            continue
        assert n <= younger, f'{body[i]}: only {younger} vector-memory operations behind the load of {breg}'
        if straight:
            assert n == younger, f'{body[i]}: {younger} vector-memory operations behind the load of {breg}'
            exact += 1
    assert exact >= 2 * 7 and bounded >= 2, (exact, bounded)  # taps 2-8 of both items; taps 0 / 1 wait for loads of the item before
