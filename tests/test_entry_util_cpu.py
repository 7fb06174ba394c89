"""csrc/entry_util.h - the call scaffolding the engine-free entries share - as plain C++ behind a main of its own: the arena layout, the
strided-view check against its definition, the sample types, the chunk of labels and the folded grid.  Enumerated cases; the expected verdicts are computed here."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'

PROGRAM = r'''
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>
static char g_msg[512];
namespace ts2d {
int fail(int code, const char* fmt, ...) {                                 // the library's is program.cpp: here the message is kept for the test
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return code;
}
}
int main(int argc, char** argv) {
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char what[16];
    while (std::fscanf(f, "%15s", what) == 1) {
        if (!std::strcmp(what, "layout")) {                                  // n, then n region sizes -> the n offsets and the total
            int n;
            if (std::fscanf(f, "%d", &n) != 1) return 3;
            ts2d::ArenaLayout lay;
            for (int i = 0; i < n; ++i) {
                unsigned long long bytes;
                if (std::fscanf(f, "%llu", &bytes) != 1) return 3;
                std::printf("%zu ", lay.add((size_t)bytes));
            }
            std::printf("%zu\n", lay.total());
        } else if (!std::strcmp(what, "view")) {                             // named, n_elems, base, 3 extents, 3 strides -> the code and the message
            int named, ext[3];
            unsigned long long n_elems;
            long long base, st[3];
            if (std::fscanf(f, "%d %llu %lld %d %d %d %lld %lld %lld", &named, &n_elems, &base, ext, ext + 1, ext + 2, st, st + 1, st + 2) != 9) return 3;
            g_msg[0] = 0;
            const int rc = ts2d::check_strided_view("entry", (size_t)n_elems, base, {ext[0], ext[1], ext[2]}, {st[0], st[1], st[2]}, named != 0);
            std::printf("%d|%s\n", rc, g_msg);
        } else if (!std::strcmp(what, "types")) {                            // per dtype: the table's size, the dispatcher's code and size
            for (int dt = 0; dt < 5; ++dt)
                ts2d::by_sample_type(dt, [&](auto t) {
                    std::printf("%zu %d %zu %d\n", ts2d::sample_size(dt), decltype(t)::dtype, sizeof(typename decltype(t)::type),
                                (int)((typename decltype(t)::type)(-1) < 0));
                });
        } else if (!std::strcmp(what, "chunk")) {                            // max_scratch_bytes, per_label, K -> L and the budget
            unsigned long long cap, per;
            int K;
            if (std::fscanf(f, "%llu %llu %d", &cap, &per, &K) != 3) return 3;
            size_t budget = 0;
            const size_t L = ts2d::labels_per_chunk((size_t)cap, (size_t)per, K, &budget);
            std::printf("%zu %zu\n", L, budget);
        } else if (!std::strcmp(what, "volume")) {
            int z, h, w;
            if (std::fscanf(f, "%d %d %d", &z, &h, &w) != 3) return 3;
            std::printf("%d\n", ts2d::volume_fits_int32(z, h, w) ? 1 : 0);
        } else if (!std::strcmp(what, "fold")) {                             // blocks, threads -> x and fold of the folded grid
            long long blocks;
            int threads;
            if (std::fscanf(f, "%lld %d", &blocks, &threads) != 2) return 3;
            const ts2d::FoldedGrid g = ts2d::fold_grid(blocks, threads);
            std::printf("%u %u\n", g.x, g.fold);
        } else {
            return 4;
        }
    }
    std::fclose(f);
    return 0;
}
'''


@pytest.fixture(scope='module')
def util_program(tmp_path_factory):
    """The header behind a main of its own, under the address and undefined-behaviour sanitizers where the toolchain links them (the compile line
    of tests/test_evaluate_cpu.py; nothing loaded into Python runs under one)."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    d = tmp_path_factory.mktemp('entry_util')
    src = d / 'util.cpp'
    src.write_text(f'#include "{os.path.join(CSRC, "entry_util.h")}"\n' + PROGRAM)
    exe = d / 'util'
    base = [cxx, '-x', 'c++', '-O1', '-g', '-std=c++17', '-Wno-unknown-pragmas', '-o', str(exe), str(src)]
    if subprocess.call(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    return str(exe)


def _run(program, tmp_path, lines):
    path = tmp_path / 'cases.txt'
    path.write_text('\n'.join(lines) + '\n')
    return subprocess.run([program, str(path)], check=True, capture_output=True, text=True).stdout.split('\n')[:-1]


LAYOUTS = [[0], [1], [255], [256], [257], [0, 0], [0, 0, 5, 0, 256, 255, 1, 0], [4096, 3, 0, 0, 1 << 33, 7], [8, 0], [1] * 13]


def test_the_layout_gives_aligned_regions_that_do_not_overlap(util_program, tmp_path):
    out = _run(util_program, tmp_path, ['layout %d %s' % (len(sizes), ' '.join(str(s) for s in sizes)) for sizes in LAYOUTS])
    assert len(out) == len(LAYOUTS)
    for sizes, line in zip(LAYOUTS, out):
        *offs, total = (int(v) for v in line.split())
        assert len(offs) == len(sizes) and offs[0] == 0 and all(o % 256 == 0 for o in offs), (sizes, offs)
        for i in range(1, len(offs)):
            assert offs[i] >= offs[i - 1] + sizes[i - 1], (sizes, offs)                      # a region starts behind the end of the one before
            assert (offs[i] > offs[i - 1]) == (sizes[i - 1] > 0), (sizes, offs)              # increasing; a zero-byte region takes no room
            assert offs[i] - (offs[i - 1] + sizes[i - 1]) < 256, (sizes, offs)               # ... and no more than the alignment is left between
        assert total >= offs[-1] + sizes[-1] and total % 256 == 0 and total - (offs[-1] + sizes[-1]) < 256, (sizes, offs, total)


EXTENTS = (3, 4, 5)
SLACK = 7


def _view_cases():
    """Every sign combination of the strides of a 3 x 4 x 5 view (20, 5 and 1 elements), in a buffer with room to spare and in one that fits
    exactly: the base at either end of the buffer, one element past either end, and a buffer one element short."""
    cases = []
    for signs in itertools.product((1, -1), repeat=3):
        strides = tuple(s * m for s, m in zip(signs, (20, 5, 1)))
        neg = -sum((e - 1) * s for e, s in zip(EXTENTS, strides) if s < 0)
        pos = sum((e - 1) * s for e, s in zip(EXTENTS, strides) if s > 0)
        assert neg + pos == 59
        for n in (60 + SLACK, 60):
            for base in (neg, neg - 1, n - 1 - pos, n - pos):
                cases.append((n, base, strides))
        cases.append((59, neg, strides))
    cases.append((1, 0, (0, 0, 0)))                                                          # a view that repeats one element
    cases.append((0, 0, (0, 0, 0)))
    return cases


def _inside(n_elems, base, extents, strides):
    touched = [base + sum(i * s for i, s in zip(idx, strides)) for idx in itertools.product(*[(0, e - 1) for e in extents])]
    lo, hi = min(touched), max(touched)
    return 0 <= lo and hi < n_elems


def test_the_view_check_is_its_definition(util_program, tmp_path):
    cases = _view_cases()
    assert len(cases) == 8 * 9 + 2
    want = [_inside(n, base, EXTENTS, strides) for n, base, strides in cases]
    assert want.count(True) == 8 * 4 + 1 and want.count(False) == 8 * 5 + 1                  # (per combination: each end of either buffer fits)
    for named in (1, 0):
        out = _run(util_program, tmp_path, ['view %d %d %d %d %d %d %d %d %d' % ((named, n, base) + EXTENTS + strides) for n, base, strides in cases])
        assert len(out) == len(cases)
        for (n, base, strides), ok, line in zip(cases, want, out):
            refusal = (f'-1|entry: the strided view (base, sz, sy, sx) leaves the buffer of n_elems {n}' if named
                       else '-1|entry: the strided view leaves the buffer')
            assert line == ('0|' if ok else refusal), (n, base, strides)


def test_the_sample_types_the_chunk_and_the_extent(util_program, tmp_path):
    chunks = [(0, 1 << 20, 255), (0, 1 << 20, 300), (0, (256 << 20) + 1, 5), (1000, 100, 255), (1000, 100, 3), (99, 100, 3), (100, 100, 3)]
    volumes = [(1, 1, 1), (0, 4, 4), (4, -1, 4), (4, 4, 0), (1, 1, 2 ** 31 - 1), (2, 1, 2 ** 30), (2 ** 16, 2 ** 15, 1), (2 ** 16, 2 ** 15 - 1, 1),
               (1291, 1291, 1289), (2 ** 15, 2 ** 15, 2)]
    out = _run(util_program, tmp_path, ['types'] + ['chunk %d %d %d' % c for c in chunks] + ['volume %d %d %d' % v for v in volumes])
    assert out[:5] == ['2 0 2 1', '1 1 1 0', '4 2 4 1', '2 3 2 0', '4 4 4 1']                # int16, uint8, float32, uint16, int32
    for (cap, per, K), line in zip(chunks, out[5:]):
        budget = cap or 256 << 20
        assert line == f'{min(budget // per, K)} {budget}', (cap, per, K)
    for (z, h, w), line in zip(volumes, out[5 + len(chunks):]):
        assert line == str(int(min(z, h, w) >= 1 and z * h <= 2 ** 31 - 1 and z * h * w <= 2 ** 31 - 1)), (z, h, w)


def test_a_folded_grid_covers_every_block_and_no_axis_passes_2_32_work_items(util_program, tmp_path):
    """Up to 2^32 - 1 work-items along x the grid is the plain one (fold 1: the launch of before); beyond, x * threads stays below 2^32, x * fold
    covers the blocks with less than one fold to spare, and the fold stays far below the 65535 of a grid's other axes."""
    cases = [(b, t) for t in (64, 256) for b in (1, 2, 1000, 2 ** 32 // t - 1, (2 ** 32 - 1) // t, 2 ** 32 // t, 2 ** 32 // t + 1, 67117056 // (t // 64),
                                                 2 ** 29, 2 ** 31 - 1)]
    out = _run(util_program, tmp_path, ['fold %d %d' % c for c in cases])
    folded = 0
    for (blocks, threads), line in zip(cases, out):
        x, fold = (int(v) for v in line.split())
        assert x * threads <= 2 ** 32 - 1 and x * fold >= blocks and x * (fold - 1) < blocks and 1 <= fold <= 129, (blocks, threads, x, fold)
        assert (fold == 1) == (blocks * threads <= 2 ** 32 - 1) and (fold > 1 or x == blocks), (blocks, threads, x, fold)
        folded += fold > 1
    assert folded >= 8
