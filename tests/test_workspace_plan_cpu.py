"""The workspace plan of csrc/dispatch.cpp (choose_all, plan_activations, workspace_layout) as properties over a sweep, on the CPU.

``ensure_workspace`` (csrc/engine.hip) keeps a layout made for ``(Bw, H, W, fw)`` and admits every later run ``(b, fr)`` with ``b <= Bw``, the same
extent, precision mode and keep flag, and ``fw or not fr``.  tests/plan_driver.cpp - the planners behind a main of their own, under the address
and undefined-behaviour sanitizers, leak checking on - takes every such (layout, run) pair of the sweep below and checks, from the Op, Tensor,
Choice and WsLayout data alone and with every consumption figure restated from the launcher or kernel that touches the region:

  W1  a buffer for every tensor the run writes: its own of at least the run's bytes, or - the output of a transposed conv only - the one
      scratch region, ``has_up`` and at most kSbkElems / 2 elements; no op without a kernel but the documented 16-bit refusals
  W2  no op writes its output over a tensor that was written earlier and is read by it or a later op (read sets of the RUN: a composed entry
      reads the coarse tensor and the skip, a fused first block the network input, a join its residual); with keep_activations no two
      tensors share a byte; the tenant of the scratch region is read by the next op only
  W3  the split-K slices, the statistics partials (those of the split-K reduce pass too) and every scale / shift vector fit their regions;
      regions 256-byte aligned, disjoint, inside the layout
  W4  the tile geometry of every Choice against the chosen kernel's own tile, staging capacity and FLEX bounds
  W5  under the full dispatch, what can change a row's bits (k, bn, ksplit, TH, TW, NIMG, flex, k32, s2p, ks, ppt, fused_stats, first_full,
      first_split, half) is the same for every batch; ``seg``, ``tiles_*``, ``n_mtiles`` (and ``npp`` / ``nch``, functions of ``k32`` and the op)
      may differ.  No other field had to be exempted.  The tile of the tile_geom family is one per op over every mode and batch.

THE SWEEP (the constants and _nets() below state it; the driver runs what the spec file spells):
  nets       the canonical net, its 7-stage form (448 x 576), the 9-stage 1024 geometry, the 4-stage (32, 64, 128, 128) net, EDGE, the
             `widths` net (16, 48, 80, 100) with its (2, 1) stage, the per-axis-stride cases of cases.SMALL_CASES, every case of RES_CASES
             (16-bit mode with "resf16" on - planned - and off - refused, enumerated)
  modes      exact, split, f16
  extents    canonical: 128 ... 1024 in steps of 128 per axis (128 x 128 leaves one bottleneck pixel and is refused), 640 x 384 among them; the
             7-stage form: every 2nd diagonal of (64, 128, 192, 320, 384, 448, 576, 640)^2, and 448 x 576 and 640 x 384 always; 9 stages:
             256 ... 1024 in steps of 256; small nets: AXIS_MULTIPLES of the net's divisor and AXIS_EXTENTS up to 640 per axis, every THIN-th
             diagonal of the index grid (_thinned: every height and every width stays in), EDGE's 96 x 160 always
  batches    Bw and b from (1, 2, 3, 4, 5, 8, 12, 16, 64, 128), both dispatch flags on either side
  settings   keep_activations on (every 2nd of those diagonals), num_cus 64 and 304 (every 3rd), and - on every 4th, with the pairs (64, 1),
             (16, 3), (5, 5) - each twin of TWINS (tests/test_gpu_full_batch_layers.py), "sbk" = 0 and "flex" = 0;
             test_the_thinning_keeps_both_axes holds every setting to as many widths as heights

Counts of the last run (printed by test_the_sweep_counts with ``pytest -s``; profiles/r33_plan_sweep.txt has them per net and mode): 219 880
plans and layouts made, 1 053 171 admitted (layout, run) pairs checked, 43 395 pairs of the 16-bit mode refused on residual encoders without
"resf16" and no other; compile 9-16 s, the sweep 55-61 s in one process.

One statement is narrower here than "NIMG > 1 implies TH == Ht and TW == Wt": the first block keeps the power-of-two tile, whose slot may exceed a
tiny image; conv3x3_first masks the rows past it (csrc/kernels_first.h), so there the check is that the image fits its slot."""
import pytest

from tests import cases
from tests import plan_driver_util as PD
from tests.resenc_util import RES_CASES
from tests.test_gpu_default_dispatch import EDGE
from tests.test_gpu_full_batch_layers import TWINS
from totalsegmentator2d_amd.arch import UNetArch

BATCHES = (1, 2, 3, 4, 5, 8, 12, 16, 64, 128)
TWIN_PAIRS = ((64, 1), (16, 3), (5, 5))
MODES = ('exact', 'split', 'f16')
AXIS_MULTIPLES = (1, 2, 3, 4, 5, 6)                               # of the net's divisor along the axis
AXIS_EXTENTS = (64, 96, 128, 160, 192, 256, 320, 384, 448, 512, 640)    # ... and these, where the divisor divides them
THIN = 5                                                          # small nets: every THIN-th diagonal of the index grid of the axis values (_thinned)
KEEP_EVERY, CUS_EVERY, TWIN_EVERY = 2, 3, 4                       # every n-th of those diagonals, for the settings beside the default
EXTRA_OPTIONS = ({'sbk': 0}, {'flex': 0})


def _thinned(arch, hs, ws, every, extras=()):
    """The pairs (hs[i], ws[j]) with (i + j) % every == 0 - diagonals of the index grid, so that every value of either axis stays in the sweep
    however far it is thinned - without the shapes that leave a single bottleneck pixel (reserve_checked refuses them: InstanceNorm needs more
    than one), and `extras` whatever the thinning."""
    dy, dx = arch.divisors
    grid = [(h, w) for i, h in enumerate(hs) for j, w in enumerate(ws) if (i + j) % every == 0 and (h // dy) * (w // dx) > 1]
    return grid + [hw for hw in extras if hw not in grid]


def _small_axes(arch):
    dy, dx = arch.divisors
    return (sorted({m * dy for m in AXIS_MULTIPLES} | {v for v in AXIS_EXTENTS if v % dy == 0}),
            sorted({m * dx for m in AXIS_MULTIPLES} | {v for v in AXIS_EXTENTS if v % dx == 0}))


def _nets():
    """name -> (arch, heights, widths, THIN of the default settings, extents that are always in): the architectures where the GPU suite defines them."""
    canonical, tsxr9 = UNetArch.canonical(), UNetArch.canonical(input_channels=1, num_classes=26, n_stages=9)
    steps, steps9, steps7 = tuple(range(128, 1025, 128)), tuple(range(256, 1025, 256)), (64, 128, 192, 320, 384, 448, 576, 640)
    nets = {'canonical': (canonical, steps, steps, 1, ()),
            'canonical7': (UNetArch.canonical(n_stages=7), steps7, steps7, 2, ((448, 576), (640, 384))),
            'tsxr9': (tsxr9, steps9, steps9, 1, ())}
    small = {'composed4': cases.unet(4, (32, 64, 128, 128), 6, cin=2),
             'edge': cases.unet(EDGE['n_stages'], EDGE['feats'], EDGE['K']),
             'widths': cases.unet(4, (16, 48, 80, 100), 5, cin=2, nconv=2, strides=[(1, 1), (2, 2), (2, 2), (2, 1)])}
    for name, case in cases.SMALL_CASES.items():
        if any(tuple(s) not in ((1, 1), (2, 2)) for s in case[0].strides):
            small[name] = case[0]
    for name, case in RES_CASES.items():
        small[name] = case[0]
    for name, arch in small.items():
        nets[name] = (arch,) + _small_axes(arch) + (THIN, ((96, 160),) if name == 'edge' else ())
    return nets


def _extents(net, times=1):
    """The extents of a net for a setting that takes every `times`-th diagonal of the default settings' extents."""
    arch, hs, ws, thin, extras = net
    return _thinned(arch, hs, ws, thin * times, extras)


def _words(kind, values):
    return kind + ' ' + ' '.join(str(v) for v in values) + ' end'


def _block(tag, options, modes, extents, pairs=None):
    lines = ['tag ' + tag, _words('set', [v for kv in options.items() for v in kv]), _words('modes', [PD.MODE_ID[m] for m in modes])]
    lines.append(_words('pairs', [v for p in pairs for v in p]) if pairs else 'pairs end')
    lines += [_words('extents', [v for hw in extents for v in hw]), 'run']
    return lines


def _settings(net):
    """[(tag, options, modes, extents, pairs or None)]: every block of the sweep for one net."""
    arch = net[0]
    residual = arch.encoder == 'residual'
    on = {'resf16': 1} if residual else {}
    every, keep, cus, twin = _extents(net), _extents(net, KEEP_EVERY), _extents(net, CUS_EVERY), _extents(net, TWIN_EVERY)
    if residual:                      # the 16-bit mode is opt-in there: planned with "resf16", refused without
        blocks = [('default', {}, ('exact', 'split'), every, None), ('resf16=1', {'resf16': 1}, ('f16',), every, None), ('resf16=0', {}, ('f16',), keep, None)]
    else:
        blocks = [('default', {}, MODES, every, None)]
    blocks.append(('keep=1', dict(on, keep=1), MODES, keep, None))
    blocks += [(f'num_cus={n}', dict(on, num_cus=n), MODES, cus, None) for n in (64, 304)]
    for opts, modes in TWINS + tuple((o, ('split', 'f16')) for o in EXTRA_OPTIONS):
        blocks.append((','.join(f'{k}={v}' for k, v in opts.items()), dict(on, **opts), modes, twin, TWIN_PAIRS))
    return blocks


def sweep_spec():
    lines = [_words('batches', BATCHES)]
    for name, net in _nets().items():
        lines.append(PD.net_words(name, net[0]))
        for block in _settings(net):
            lines += _block(*block)
    return lines


def test_the_thinning_keeps_both_axes():
    """The default settings of every net visit every height and every width of the net's axes, and every other setting as many widths as
    heights, at least half of them (a stride through the row-major product would collapse one axis)."""
    for name, net in _nets().items():
        _, hs, ws, _, _ = net
        for tag, _, _, extents, _ in _settings(net):
            assert len(set(extents)) == len(extents) >= 3, (name, tag)
            seen_h, seen_w = {h for h, _ in extents}, {w for _, w in extents}
            if tag in ('default', 'resf16=1'):
                assert seen_h >= set(hs) and seen_w >= set(ws), (name, tag, sorted(set(hs) - seen_h), sorted(set(ws) - seen_w))
            assert abs(len(seen_h) - len(seen_w)) <= 2 and min(len(seen_h), len(seen_w)) >= min(len(hs), len(ws)) // 2, (name, tag, sorted(seen_h), sorted(seen_w))


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return PD.build(tmp_path_factory.mktemp('plan_driver'))


def _run(driver, tmp_path, lines, what, tamper=0):
    path = tmp_path / 'spec.txt'
    path.write_text('\n'.join(lines) + '\n')
    return PD.run(driver, ['ws', path] + (['--tamper', tamper] if tamper else []), what)


def _tally(out):
    assert out[-1].startswith('tally '), out[-3:]
    return {k: int(v) for k, v in (w.split('=') for w in out[-1].split()[1:])}


@pytest.fixture(scope='module')
def sweep(driver, tmp_path_factory):
    return _run(driver, tmp_path_factory.mktemp('sweep'), sweep_spec(), 'sweep')


def test_no_admitted_pair_of_the_sweep_violates_a_property(sweep):
    viol = [line for line in sweep if line.startswith('viol ')]
    tally = _tally(sweep)
    assert not viol and not any(tally[p] for p in ('W1', 'W2', 'W3', 'W4', 'W5')), (tally, viol[:20])
    assert not [line for line in sweep if line.startswith('skip ')], 'every extent of the sweep is one reserve_checked admits'


def test_the_sweep_counts(sweep):
    """Every block of the sweep ran pairs (or, for the 16-bit mode on a residual encoder without "resf16", refused all of them); the totals."""
    counts = [dict(w.split('=') for w in line.split()[4:]) | {'net': line.split()[1], 'mode': line.split()[2][5:], 'tag': line.split()[3]}
              for line in sweep if line.startswith('count ')]
    assert counts
    per = {}
    for c in counts:
        pairs, refused, layouts = int(c['pairs']), int(c['refused']), int(c['layouts'])
        if c['tag'] == 'resf16=0':
            assert pairs == 0 and refused > 0, c                  # the documented refusal, enumerated
        else:
            assert pairs > 0 and refused == 0, c
        k = (c['net'], c['mode'])
        per[k] = tuple(a + b for a, b in zip(per.get(k, (0, 0, 0)), (layouts, pairs, refused)))
    for (net, mode), (layouts, pairs, refused) in sorted(per.items()):
        print(f'{net:12s} {mode:5s} layouts {layouts:7d} pairs {pairs:8d} refused {refused:6d}')
    print('total: layouts %d pairs %d refused %d; compile %.1f s, sweep %.1f s' % (
        sum(v[0] for v in per.values()), sum(v[1] for v in per.values()), sum(v[2] for v in per.values()), PD.TIMES['compile'], PD.TIMES['sweep']))
    assert set(n for n, _ in per) == set(_nets())


# ------------------------------------------------------------------------------------------------------------------ what the sweep found
# Tiles of several tiny images.  tile_geom returned the power-of-two tile without holding it to the staging budget: 16 images of 2 x 8 (or
# 8 x 2) pixels are 16 x 4 x 10 = 640 patch pixels where conv_mfma_f32 at 16-channel chunks stages 576 (exact mode; kernels.h:132-133, 190-201),
# and 8 images of 1 x 32 are 8 x 3 x 34 = 816 where conv3x3_f16x3 stages 640 (split and 16-bit mode; kernels_f16x3.h:294-298) - the last images
# of such a tile (from the 15th and the 7th slice of a batch on) read LDS nobody wrote.  W4 reported both at the commit before the fix in
# csrc/dispatch.cpp (tile_geom).  The smallest cases, by name: the 4-stage (32, 64, 128, 128) net on 16 x 64, 64 x 16 and 8 x 256.
TINY_TILE_CASES = ((16, 64), (64, 16), (8, 256))


def test_tiles_of_several_tiny_images_fit_what_the_kernels_stage(driver, tmp_path):
    arch = cases.unet(4, (32, 64, 128, 128), 6, cin=2)
    lines = [_words('batches', (1, 8, 16)), PD.net_words('composed4', arch)] + _block('tiny-tiles', {}, MODES, TINY_TILE_CASES)
    out = _run(driver, tmp_path, lines, 'tiny tiles')
    assert not [line for line in out if line.startswith('viol ')], out[:10]
    assert all(v == 0 for v in _tally(out).values())


# ------------------------------------------------------------------------------------------------------------------ the per-image limit
# reserve_checked (csrc/engine.hip) refuses an extent whose widest per-image plane - the widest activation tensor or the NCHW input, at four bytes
# per element in every mode - passes 2^31 - 1 bytes (csrc/program.cpp: image_extent_ok; DESIGN.md, "32-bit quantities of the forward path").
# (name, net, mode, H, bytes per level-0 pixel of the widest plane): W = limit is the largest multiple of the divisor with H * W * bytes <= 2^31 - 1.
LIMIT_CASES = (('w32', cases.unet(2, (32, 32), 1, cin=1, nconv=1), 'split', 4096, 32 * 4),          # widths of 32, float32 storage
               ('w32-exact', cases.unet(2, (32, 32), 1, cin=1, nconv=1), 'exact', 4096, 32 * 4),
               ('w24', cases.unet(2, (24, 24), 1, cin=1, nconv=1), 'split', 4096, 32 * 4),          # a width the engine pads to 32: the plane is the padded one
               # half storage: the SAME limit - the dispatch guards every per-image kernel with fits32(pixels * C * 4) whatever the mode stores
               # (csrc/dispatch.cpp), and the workspace plan sizes every buffer for floats
               ('w32-half', cases.unet(2, (32, 32), 1, cin=1, nconv=1), 'f16', 4096, 32 * 4),
               ('deep512', cases.unet(2, (32, 512), 2, cin=1, nconv=1), 'split', 2048, 512 * 4 // 4),   # level 1 is the widest: 512 channels on a quarter of the pixels
               ('cin64', cases.unet(2, (32, 32), 1, cin=64, nconv=1), 'f16', 2048, 64 * 4))         # the float32 NCHW input is the widest


@pytest.mark.parametrize('name,arch,mode,H,per_px', LIMIT_CASES, ids=[c[0] for c in LIMIT_CASES])
def test_the_per_image_limit_at_below_and_above(driver, tmp_path, name, arch, mode, H, per_px):
    limit = (2 ** 31 - 1) // (H * per_px) // 2 * 2                    # W is a multiple of the divisor 2
    assert H * limit * per_px <= 2 ** 31 - 1 < H * (limit + 2) * per_px
    lines = [PD.net_words(name, arch)] + [f'limit {PD.MODE_ID[mode]} {H} {w}' for w in (limit - 2, limit, limit + 2)] + [f'limits {PD.MODE_ID[mode]}']
    out = _run(driver, tmp_path, lines, f'limit {name}')
    got = [dict(w.split('=') for w in line.split()[2:]) for line in out if line.startswith('limit ')]
    assert [(int(g['W']), int(g['ok']), int(g['bytes'])) for g in got] == [(w, int(w <= limit), H * w * per_px) for w in (limit - 2, limit, limit + 2)], got
    assert all(int(g['call']) == 2 ** 31 for g in got)                # pixels per call: 2^31 on a plain encoder ...
    sweep =[line for line in out if line.startswith('limits ')]
    assert len(sweep) == 1 and sweep[0].endswith('viol=0') and int(sweep[0].split()[3].split('=')[1]) > 100, (sweep, [line for line in out if line.startswith('viol ')])


def test_the_per_call_pixel_limit_of_a_residual_encoder(driver, tmp_path):
    """... and 2^29 - 32 on a residual encoder: res_join launches 256 threads per 32 pixels of a level (csrc/engine.hip launch_join, float32 storage)
    and a launch holds fewer than 2^32 threads."""
    ppb, threads, most = 32, 256, 2 ** 29 - 32
    assert (most + ppb - 1) // ppb * threads < 2 ** 32 <= (most + 1 + ppb - 1) // ppb * threads
    out = _run(driver, tmp_path, [PD.net_words('res_min', RES_CASES['res_min'][0]), f'limit {PD.MODE_ID["split"]} 256 256'], 'call limit')
    got = [dict(w.split('=') for w in line.split()[2:]) for line in out if line.startswith('limit ')]
    assert len(got) == 1 and int(got[0]['call']) == most + 1 and int(got[0]['ok']) == 1, got


# ------------------------------------------------------------------------------------------------------------------ the proof that it bites
# The named case: the EDGE net on 96 x 160 (ragged deep levels), split mode, a layout reserved for 5 slices under the full dispatch, a run of
# one slice under the by-size dispatch - split-K convs, an un-composed decoder entry in the scratch region, extent-following tiles.
def _named_case():
    arch = cases.unet(EDGE['n_stages'], EDGE['feats'], EDGE['K'])
    return [_words('batches', (1, 3, 5)), PD.net_words('edge', arch)] + _block('named', {}, ('split',), [(96, 160)])


DAMAGES = ((1, 'W3', 'the split-K region one 256-byte block short'), (2, 'W2', 'an output moved onto a live tensor'), (3, 'W1', 'has_up cleared'),
           (4, 'W1', "a tensor's size one block short"), (5, 'W4', 'a tile one row short of its level'), (6, 'W5', 'a split factor doubled at b = 1 only'))


def test_the_named_case_is_clean(driver, tmp_path):
    out = _run(driver, tmp_path, _named_case(), 'named')
    assert not [line for line in out if line.startswith('viol ')], out
    assert _tally(out) == {'W1': 0, 'W2': 0, 'W3': 0, 'W4': 0, 'W5': 0, 'tampered': 0}


@pytest.mark.parametrize('tamper,prop,what', DAMAGES)
def test_each_damage_to_the_planners_data_is_reported_under_its_property(driver, tmp_path, tamper, prop, what):
    out = _run(driver, tmp_path, _named_case(), f'tamper {tamper}', tamper=tamper)
    tally = _tally(out)
    assert tally['tampered'] > 0, (what, 'the named case has nothing to damage', tally)
    assert tally[prop] > 0 and any(line.startswith(f'viol {prop} edge mode=split H=96 W=160') for line in out), (what, tally, out[:10])
    others = {p: n for p, n in tally.items() if p not in (prop, 'tampered') and n}
    assert not others, (what, 'reported under another property too', others, [line for line in out if line.startswith('viol ')][:10])
