"""Register / scratch / LDS table of every kernel instantiation in libts2d_engine.so's device code ("report VGPR / AGPR /
scratch per instantiation").  Runs in the build container (hipcc cross-compiles without a GPU):

    python scripts/kernel_resources.py [profiles/r06_resources.txt]
    python scripts/kernel_resources.py --identity <csrc of another checkout> [profiles/r13_kernel_identity.txt]

Compiles every csrc/*.hip to gfx950 assembly with the Makefile's device flags and reads the amdhsa metadata hipcc writes per kernel
(the same numbers `llvm-readelf --notes` prints for the code object): arch VGPRs, AGPRs, SGPRs, spilled registers, scratch bytes per
lane, static LDS, max workgroup size -> waves per SIMD the register file allows (512 registers per SIMD lane: 2 waves at <= 256).

--identity compares the device code of this tree with another checkout's, function by function under its mangled name: the body from
its label to .Lfunc_end without comments and blank lines, `.LBB<n>_` rewritten to `.LBB_` (n is the function's index in its unit: the
only thing a move between units may change), and its .amdhsa_kernel block.  Exit status 1 unless both trees hold the same names, each
in exactly one unit, with equal bodies and blocks."""
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
FILT = 'c++filt'


def device_asm(csrc):
    """{unit: gfx950 assembly} of every .hip in `csrc`, compiled with the device flags of its own Makefile"""
    devflags = subprocess.check_output(['make', '-s', '-C', csrc, 'flags'], text=True).split()
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for src in sorted(glob.glob(os.path.join(csrc, '*.hip'))):
            s = os.path.join(td, 'unit.s')
            subprocess.check_call([HIPCC, '-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-S', *devflags, '-o', s, src],
                                  stderr=subprocess.DEVNULL)
            out[os.path.basename(src)] = open(s).read()
    return out


def functions(units):
    """{mangled name: [(unit, body, .amdhsa_kernel block)]} over the units of one tree"""
    found = {}
    for unit, asm in units.items():
        for name in re.findall(r'^\s*\.type\s+(\w+),@function', asm, re.M):
            start = asm.index(f'\n{name}:') + 1
            text = asm[asm.index('\n', start) + 1:asm.index('\n.Lfunc_end', start)]
            body = [re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0].rstrip()) for ln in text.split('\n')]
            k = re.search(rf'^\s*\.amdhsa_kernel {name}\n(.*?)^\s*\.end_amdhsa_kernel', asm, re.M | re.S)
            found.setdefault(name, []).append((unit, [ln for ln in body if ln.strip()], k.group(1) if k else None))
    return found


def identity(other_csrc, out_path):
    old, new = functions(device_asm(other_csrc)), functions(device_asm(CSRC))
    lines = [f'# scripts/kernel_resources.py --identity: device code of csrc/*.hip against another checkout, gfx950, Makefile device flags',
             f'# functions: {len(old)} there, {len(new)} here; bodies from label to .Lfunc_end (comments dropped, .LBB<n>_ -> .LBB_) and .amdhsa_kernel blocks',
             f'{"function":<72} {"unit":<11} {"lines":>6} {"body":>6} {"kernel block":>12}']
    bad = sorted(set(old) ^ set(new))
    for name in bad:
        lines.append(f'{name[:72]:<72} only {"there" if name in old else "here"}')
    for name in sorted(set(old) & set(new)):
        (_, b0, k0), (unit, b1, k1) = old[name][0], new[name][0]
        once = len(old[name]) == 1 and len(new[name]) == 1
        same_b, same_k = b0 == b1, k0 == k1
        if not (once and same_b and same_k):
            bad.append(name)
        lines.append(f'{name[:72]:<72} {unit if once else "SEVERAL":<11} {len(b1):>6} {"equal" if same_b else "DIFFER":>6} '
                     f'{("equal" if same_k else "DIFFER") if k1 is not None or k0 is not None else "-":>12}')
    lines.append(f'# {"IDENTICAL" if not bad else "NOT IDENTICAL"}: {len(set(old) & set(new)) - len([n for n in bad if n in old and n in new])} of {len(old)} '
                 f'functions equal in body and kernel block, {len(bad)} differ or are missing')
    text = '\n'.join(lines) + '\n'
    if out_path:
        open(out_path, 'w').write(text)
    print(text)
    return 1 if bad else 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--identity':
        sys.exit(identity(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None))
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rows = []
    for unit, asm in device_asm(CSRC).items():
        meta = asm[asm.index('amdhsa.kernels:'):]
        for blk in re.split(r'\n  - \.', meta)[1:]:
            def get(key, default='0'):
                m = re.search(r'\.' + key + r':\s*(\S+)', '.' + blk)
                return m.group(1) if m else default
            name = get('name', '?')
            rows.append(dict(name=name, vgpr=int(get('vgpr_count')), agpr=int(get('agpr_count')), sgpr=int(get('sgpr_count')),
                             vspill=int(get('vgpr_spill_count')), sspill=int(get('sgpr_spill_count')),
                             scratch=int(get('private_segment_fixed_size')), lds=int(get('group_segment_fixed_size')),
                             wg=int(get('max_flat_workgroup_size'))))
    names = subprocess.check_output([FILT], input='\n'.join(r['name'].replace('DF16_', 'Dh') for r in rows), text=True).split('\n')
    for r, n in zip(rows, names):
        n = re.sub(r'^void ts2d::', '', n)
        n = re.sub(r'\(.*\)$', '', n)
        r['pretty'] = n.replace('(anonymous namespace)::', '').replace('half', '_Float16')      # (binutils' c++filt does not know DF16_: fed as Dh)
    rows.sort(key=lambda r: r['pretty'])
    lines = ['# scripts/kernel_resources.py: amdhsa metadata of every kernel in csrc/*.hip, gfx950, Makefile device flags',
             '# vgpr = architectural VGPRs (incl. the AGPR half when used), waves/SIMD = floor(512 / max(vgpr, 1)) capped at 8;',
             '# vspill / sspill = spilled vector / scalar registers, scratch = bytes per lane, lds = static bytes (dynamic LDS is set at launch)',
             f'{"kernel":<64} {"vgpr":>5} {"agpr":>5} {"sgpr":>5} {"vspill":>6} {"sspill":>6} {"scratch":>8} {"lds":>7} {"wg":>5} {"waves/SIMD":>10}']
    for r in rows:
        waves = min(8, 512 // max(r['vgpr'], 1))
        lines.append(f'{r["pretty"][:64]:<64} {r["vgpr"]:>5} {r["agpr"]:>5} {r["sgpr"]:>5} {r["vspill"]:>6} {r["sspill"]:>6} {r["scratch"]:>8} {r["lds"]:>7} {r["wg"]:>5} {waves:>10}')
    text = '\n'.join(lines) + '\n'
    if out_path:
        open(out_path, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
