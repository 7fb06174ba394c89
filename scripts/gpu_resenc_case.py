"""Per-op times of a ResEnc-M-like 2-D net on one MI355X, per precision mode: what the residual blocks' own kernels (res_join, pool_proj1x1 and
their fp16-storage instances) cost beside the 3x3 work, and what the 16-bit mode gains on such a net.  7 stages, features (32, 64, 128, 256,
512, 512, 512), blocks (1, 3, 4, 6, 6, 6, 6), one conv per decoder stage, 2 input channels, K = 18, B = 64 at 512 x 512, synthetic weights
and input resident in HBM.  Split mode and 16-bit mode (option "resf16") run in ONE process on one engine, one after the other.

    python scripts/gpu_resenc_case.py [profiles/r24_resenc_f16_case.txt] [--batch 64] [--precisions split,f16]

Times are HIP events around every launch (Engine.set_profiling), the median of 5 profiled forwards after 2 warm-up ones, per mode.  The
join's bytes are what it must move (conv2 in, the residual's window in, the sum out, 4 or 2 bytes each); the projection's FLOPs are 2 M Cin Cout."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                    # noqa: E402
from totalsegmentator2d_amd.arch import UNetArch, OP_PROJ1X1, OP_JOIN             # noqa: E402
from totalsegmentator2d_amd import weights                     # noqa: E402
from totalsegmentator2d_amd.engine import Engine               # noqa: E402

HBM_COPY_TBS = 4.9          # profiles/r02_hbm_probe.txt: copy 4.65 ... 4.94 TB/s, read 6.3, write 5.5


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    out_path = args[0] if args else None
    B = int(sys.argv[sys.argv.index('--batch') + 1]) if '--batch' in sys.argv else 64
    H = W = 512
    feats, blocks = (32, 64, 128, 256, 512, 512, 512), (1, 3, 4, 6, 6, 6, 6)
    n = len(feats)
    arch = UNetArch(input_channels=2, num_classes=18, n_stages=n, features_per_stage=feats, kernel_sizes=((3, 3),) * n,
                    strides=((1, 1),) + ((2, 2),) * (n - 1), n_conv_per_stage=(1,) * n, n_conv_per_stage_decoder=(1,) * (n - 1),
                    encoder='residual', n_blocks_per_stage=blocks)
    modes = (sys.argv[sys.argv.index('--precisions') + 1] if '--precisions' in sys.argv else 'split,f16').split(',')
    e = Engine(arch, weights.pack_blob(arch, weights.synthetic_state_dict(arch, 19)), options={'resf16': 1})
    x = torch.randn(B, 2, H, W, device='cuda')
    mask = torch.empty(B, 18, H, W // 32, dtype=torch.int32, device='cuda')
    run = lambda: e.forward(x, logits=False, mask=True, out_mask=mask)
    ms, kern = {}, {}
    for mode in modes:
        e.set_precision(mode)
        e.reserve(B, H, W)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        e.set_profiling(True)
        samples = []
        for _ in range(5):
            run()
            torch.cuda.synchronize()
            samples.append(e.op_times())
        kern[mode] = e.op_kernels()
        e.set_profiling(False)
        ms[mode] = {k: statistics.median(s[k] for s in samples) for k in samples[0]}
    total = {m: sum(ms[m].values()) for m in modes}
    prog = {o['name']: o for o in arch.program()}
    flops = arch.work(H, W)['flops'] * B
    lines = [f'# scripts/gpu_resenc_case.py: ResEnc-M-like 2-D net, features {feats}, blocks {blocks}, B = {B}, {H} x {W}, {torch.cuda.get_device_name(0)}',
             '# median of 5 profiled forwards per precision mode, both modes in one process']
    for m in modes:
        lines.append(f'# {m:<5}: sum of the launches {total[m]:.3f} ms = {B / total[m] * 1e3:.1f} slices/s; {flops / total[m] / 1e9:.1f} TFLOP/s algorithmic')
    if 'split' in modes and 'f16' in modes:
        lines.append(f'# f16 / split: {total["split"] / total["f16"]:.2f}x the slices/s ({total["f16"] / total["split"]:.3f} of the time)')
    names = list(dict.fromkeys(n for m in modes for n in ms[m]))          # (a launch may exist in one mode only: composition differs)
    lines.append(f'{"launch":<22} ' + ' '.join(f'{"kernel (" + m + ")":<24} {"ms":>8} {"share":>7}' for m in modes) + '  note (per mode)')
    fam = {m: {'res_join': 0.0, 'pool_proj1x1': 0.0, 'pool_proj1x1 statistics': 0.0} for m in modes}
    for name in names:
        op = prog.get(name)
        cols, notes = [], []
        for m in modes:
            t = ms[m].get(name)
            if t is None:
                cols.append(f'{"-":<24} {"-":>8} {"-":>7}')
                continue
            eb = 2 if m == 'f16' else 4
            if op is not None and op['op'] == OP_JOIN:
                h, w = arch.extent(op['level'], H, W)
                win = op['stride'][0] * op['stride'][1]
                nbytes = B * h * w * op['cout'] * eb * (2 + win)
                notes.append(f'{nbytes / t / 1e9:.2f} TB/s of {HBM_COPY_TBS} (copy)')
                fam[m]['res_join'] += t
            elif op is not None and op['op'] == OP_PROJ1X1:
                h, w = arch.extent(op['level'], H, W)
                fl = 2.0 * B * h * w * op['cin'] * op['cout']
                notes.append(f'{fl / t / 1e9:.1f} TFLOP/s')
                fam[m]['pool_proj1x1'] += t
            elif name.endswith('.proj.stats'):
                fam[m]['pool_proj1x1 statistics'] += t
            cols.append(f'{kern[m].get(name, ""):<24} {t:8.3f} {t / total[m]:7.2%}')
        lines.append(f'{name:<22} ' + ' '.join(cols) + '  ' + ' | '.join(notes))
    for m in modes:
        lines.append(f'# {m}: shares of the forward: ' + ', '.join(f'{k} {v:.3f} ms = {v / total[m]:.2%}' for k, v in fam[m].items()))
    slower = [n for n in names if 'split' in modes and 'f16' in modes and n in ms['split'] and n in ms['f16'] and ms['f16'][n] > ms['split'][n]]
    if 'split' in modes and 'f16' in modes:
        lines.append('# launches slower in the 16-bit mode than in the split mode: ' + (', '.join(f'{n} ({ms["split"][n]:.3f} -> {ms["f16"][n]:.3f} ms)' for n in slower) or 'none'))
    text = '\n'.join(lines) + '\n'
    print(text)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(text)
    e.close()


if __name__ == '__main__':
    main()
