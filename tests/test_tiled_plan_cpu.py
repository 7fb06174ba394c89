"""The sliding-window plan of csrc/tiled_plan.cpp (plan_tiled, rs_plan_segment) as properties, on the CPU: tests/plan_driver.cpp plans the
scenarios of scripts/tiled_plan_record.py (restated in the driver, the script's record is untouched) under the address and undefined-behaviour
sanitizers, leak checking on, and checks every accepted SwPlan from its data alone:

  T1  the regions of the scratch are 256-byte aligned, in order and hold what the chunk loop of predict_tiled_impl (csrc/tiled.hip) puts there;
      the parts of the table blob are ordered, 8-byte aligned where their structs are, inside the blob, and hold the images' tile origins
  T2  every (image, tile, variant) row is in exactly one chunk, ascending per image; batch_row + n_rows <= cap_rows <= kSwChunkRows; an image
      is aggregated in the chunk that holds its last rows and nowhere else; first blocks are the exclusive prefix sums of the segments' blocks
      and sw_find_seg's search, replayed for every block, finds the owner
  T3  sw_gather and sw_aggregate replayed lane by lane in integers: every read inside the image's floats, its rows of the batch and of the
      tile logits, every write inside the image's outputs and exactly once, 16-byte accesses 16-byte aligned (the mirrored ``src + pw - 4 - x0``
      among them), outputs of different images disjoint
  T4  tail segments: block0 are prefix sums of what sw_resample_threshold / sw_labelmap / sw_probabilities walk, destinations disjoint and inside
      rs_elems / prob_elems, tap indices inside the source rectangle, w0 + w1 == 1 exactly, w1 in [0, 1) (the coordinate is not clamped, floor()
      keeps the weight there), the taps equal ``preprocess.linear_axis_taps`` bit for bit, tap0 == -1 exactly for an un-resampled image of a
      label-map / regions / probabilities tail

Scenarios: every tail kind (none, export, label map, regions, probabilities in three modes, probability runs) x F in (1, 3) x mirror masks 0-3 x
nine image sets - among them an image of 160 rows (more than kSwChunkRows), chunks that fill exactly (2 x 32 and 1 x 64 rows), sets whose
every image is un-resampled (a tail without a single tap: the null-pointer memcpy that the record script once found) - and patches of 24 x 40,
32 x 31 and 30 x 26 on row pitches 32, 48, 100 (multiples of 4) and 70.  Last run: 988 plans, 976 of them replayed lane by lane (40 million
lanes planned, the replay takes the plans of at most 400 000), 278 calls of the record script's refusal list (232 refused, 46 that
their kind accepts because the fault is in a field it does not read); compile 9 s, run 3 s."""
import struct

import numpy as np
import pytest

from tests import plan_driver_util as PD
from totalsegmentator2d_amd import preprocess

N_PLANS, N_REFUSED = 988, 278                    # (N_REFUSED: the record script's refused calls, the ones a kind accepts among them)


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return PD.build(tmp_path_factory.mktemp('plan_driver'))


@pytest.fixture(scope='module')
def record(driver):
    return PD.run(driver, ['tiled'], 'tiled')


def _tally(out):
    assert out[-1].startswith('tally '), out[-3:]
    return {k: int(v) for k, v in (w.split('=') for w in out[-1].split()[1:])}


def test_every_accepted_plan_holds_the_properties(record):
    viol = [line for line in record if line.startswith('viol ')]
    tally = _tally(record)
    print(tally, 'compile %.1f s, run %.1f s' % (PD.TIMES['compile'], PD.TIMES['tiled']))
    assert not viol, viol[:20]
    assert all(tally[p] == 0 for p in ('T0', 'T1', 'T2', 'T3', 'T4')), tally      # T0: a scenario that should plan was refused
    assert tally['plans'] == N_PLANS and tally['refused'] == N_REFUSED and tally['replayed'] >= 970, tally


def test_the_taps_are_numpys_bit_for_bit(record):
    lines = [line.split() for line in record if line.startswith('taps ')]
    assert len(lines) >= 10
    seen = set()
    for w in lines:
        n_in, n_out, origin = int(w[1]), int(w[2]), int(w[3])
        seen.add((n_in > n_out) - (n_in < n_out))
        vals = w[4:]
        assert len(vals) == 4 * n_out, (n_in, n_out)
        i0, i1, w0, w1 = preprocess.linear_axis_taps(n_in, n_out)
        for o in range(n_out):
            got = (vals[4 * o], vals[4 * o + 1], int(vals[4 * o + 2]), int(vals[4 * o + 3]))
            want = (struct.pack('>d', float(w0[o])).hex(), struct.pack('>d', float(w1[o])).hex(), origin + int(i0[o]), origin + int(i1[o]))
            assert got == want, (n_in, n_out, origin, o, got, want)
    assert seen == {-1, 0, 1}                      # up, same size (an export resamples it all the same), down


WHAT = {1: 'export', 2: 'labelmap', 3: 'regions', 4: 'probabilities', 5: 'probabilities'}
# refusal -> (image the message names, the message; {w}: the tail's name); None: no image in front (a fault of the call, not of an image)
REFUSALS = {
    'bad patch': (None, 'entry: bad patch 0x32'),
    'bad patch + null outputs': (None, 'entry: bad patch -1x32'),
    '2^28 network rows': (None, 'entry: 268435456 network rows in one call'),
    'null image': (1, 'null image or tile pointer'),
    'null tiles': (1, 'null image or tile pointer'),
    'null tiles and too many': (0, 'null image or tile pointer'),
    'no padded output': (2, 'both outputs are null'),
    'no tiles': (1, 'bad tiling: 0 tiles of 32x32 on 32x48'),
    'patch above image': (0, 'bad tiling: 2 tiles of 32x32 on 31x32'),
    'too many tiles': (0, 'bad tiling: 1048577 tiles of 32x32 on 40x32'),
    '2^31 elements': (1, '32768x32768 exceeds 2^31 elements per image'),
    'tile leaves': (2, 'tile 1 at (19,5) leaves the 50x70 image'),           # the form tests/test_gpu_tiled_batch.py greps for
    'null outputs': (1, '{w}: {null}'),
    'null outputs + rect leaves': (1, '{w}: {null}'),
    'rect leaves': (2, '{w}: source rectangle 50x60 at (1,2) is empty or leaves the 50x70 image'),
    'rect negative': (0, '{w}: source rectangle 30x32 at (4,-1) is empty or leaves the 40x32 image'),
    'rect empty': (0, '{w}: source rectangle 30x0 at (4,0) is empty or leaves the 40x32 image'),
    'bad out extent': (1, '{w}: bad output extent 0x33'),
    'bad out at 0 + no tiles at 1': (0, '{w}: bad output extent 45x-4'),
    '2^31 outputs': (1, '{w}: 65536x32768 exceeds 2^31 output elements'),
    'box negative': (1, '{w}: the 32x33 output at (-1,1) leaves the full extent 40x36'),
    'box leaves': (1, '{w}: the 32x33 output at (3,1) leaves the full extent 40x33'),
    'full empty': (1, '{w}: the 32x33 output at (3,1) leaves the full extent 0x36'),
    '2^31 full': (2, '{w}: 3 x 32768x32768 exceeds 2^31 output elements'),
    'null first output': (1, '{w}: the output is null'),
    'null second output': (1, '{w}: the output is null'),
    '2^30 outputs': (1, '{w}: 32768x32768 exceeds 2^31 output elements'),
    'rect leaves at 0 + null outputs at 1': (0, '{w}: source rectangle 99x32 at (4,0) is empty or leaves the 40x32 image'),
    'no tiles + bad out, both at 0': (0, 'bad tiling: 0 tiles of 32x32 on 40x32'),
    'bad out + full empty': (1, '{w}: bad output extent 0x33'),
    'rect leaves + box negative': (1, '{w}: source rectangle 32x33 at (100,8) is empty or leaves the 32x48 image'),
    'rect empty at 62 (below 2^28 rows)': (62, '{w}: source rectangle 0x32 at (4,0) is empty or leaves the 40x32 image'),
    'runs null image': ((0, 1), 'null image or tile pointer'),
    'runs rect leaves': ((1, 2), '{w}: source rectangle 40x33 at (0,8) is empty or leaves the 32x48 image'),
    'runs full empty': ((0, 0), '{w}: the 32x33 output at (3,1) leaves the full extent 0x36'),
    'runs no tiles at 0 + box leaves in run 1': ((0, 0), 'bad tiling: 0 tiles of 32x32 on 32x48'),
}
# ... where the kind's message differs (a probabilities image is measured by its full extent)
OTHERWISE = {('2^30 outputs', 4): (1, '{w}: 3 x 65536x65536 exceeds 2^31 output elements')}
# The fault is in a field the kind does not read - the padded outputs of a call that has a tail, the output the kind does not have (an export needs
# one of two, a label map the uint8 plane, probabilities the float planes), the full extent and the box of a tail that is no probabilities tail, 2^30
# elements of ONE plane - so the call is accepted: rc 0 and a plan with chunks
ACCEPTED = {'no padded output': (1, 2, 3, 4), 'null first output': (1, 4), 'null second output': (1, 2, 3), '2^30 outputs': (2, 3),
            'box negative': (1, 2, 3), 'box leaves': (1, 2, 3), 'full empty': (1, 2, 3), '2^31 full': (1, 2, 3)}


def test_every_refused_call_says_why_and_leaves_no_chunks(record):
    lines = [line.split('|') for line in record if line.startswith('refused|')]
    assert len(lines) == N_REFUSED
    names, accepted = set(), 0
    for _, name, kind, named, rc, chunks, msg in lines:
        kind, named = int(kind), int(named)
        names.add(name)
        if kind in ACCEPTED.get(name, ()):
            accepted += 1
            assert int(rc) == 0 and int(chunks) >= 1 and msg == '', (name, kind, rc, chunks, msg)
            continue
        assert int(rc) == -1 and int(chunks) == 0, (name, kind, rc, chunks)
        if name == '2^26 taps':                  # (a probabilities image of 2^25 rows is past 2^31 elements of its full extent before the taps are counted)
            assert 'more than 2^26 output rows + columns in one call' in msg or (kind == 4 and 'exceeds 2^31 output elements' in msg), (kind, msg)
            continue
        image, text = OTHERWISE.get((name, kind), REFUSALS[name])
        text = text.format(w=WHAT.get(kind, ''), null='both outputs are null' if kind == 1 else 'the output is null')
        if image is None or not named:
            pre = ''
        elif isinstance(image, tuple):
            pre = 'run %d: image %d: ' % image
        else:
            pre = 'image %d: ' % image
        assert msg == pre + text, (name, kind, named, msg)
    assert names == set(REFUSALS) | {'2^26 taps'} and accepted == 2 * sum(len(v) for v in ACCEPTED.values())


# ------------------------------------------------------------------------------------------------------------------ the proof that it bites
DAMAGES = ((7, 'T2', 'cap_rows one row short of the largest chunk'), (8, 'T3', "the last image's outputs moved onto the image before it"),
           (9, 'T2', 'the last image never aggregated'), (10, 'T1', 'the tile logits one block into the batch'))


@pytest.mark.parametrize('tamper,prop,what', DAMAGES)
def test_each_damage_to_a_plan_is_reported_under_its_property(driver, tamper, prop, what):
    out = PD.run(driver, ['tiled', '--tamper', tamper], f'tiled tamper {tamper}')
    tally = _tally(out)
    assert tally[prop] > 0 and any(line.startswith(f'viol {prop} ') for line in out), (what, tally)
