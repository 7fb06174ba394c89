"""Per-op times of a ResEnc-M-like 2-D net on one MI355X: what the residual blocks' own kernels (res_join, pool_proj1x1) cost beside the
3x3 work.  7 stages, features (32, 64, 128, 256, 512, 512, 512), blocks (1, 3, 4, 6, 6, 6, 6), one conv per decoder stage, 2 input
channels, K = 18, B = 64 at 512 x 512, split mode, synthetic weights and input resident in HBM.

    python scripts/gpu_resenc_case.py [profiles/r19_resenc_ops.txt] [--batch 64]

Times are HIP events around every launch (Engine.set_profiling), the median of 5 profiled forwards after 2 warm-up ones.  The join's
bytes are what it must move (conv2 in, the residual's window in, the sum out, fp32); the projection's FLOPs are 2 M Cin Cout."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                    # noqa: E402
from totalsegmentator2d_amd.arch import UNetArch, OP_PROJ1X1, OP_JOIN             # noqa: E402
from totalsegmentator2d_amd import weights                     # noqa: E402
from totalsegmentator2d_amd.engine import Engine               # noqa: E402

HBM_COPY_TBS = 4.9          # profiles/r02_hbm_probe.txt: copy 4.65 ... 4.94 TB/s, read 6.3, write 5.5
F32_MFMA_TFS = 155.0        # measured peak of v_mfma_f32_32x32x2_f32 on the MI355X; an untuned LDS-tiled 4096^3 GEMM on it reaches 122


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
    e = Engine(arch, weights.pack_blob(arch, weights.synthetic_state_dict(arch, 19)))
    x = torch.randn(B, 2, H, W, device='cuda')
    mask = torch.empty(B, 18, H, W // 32, dtype=torch.int32, device='cuda')
    e.reserve(B, H, W)
    run = lambda: e.forward(x, logits=False, mask=True, out_mask=mask)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    e.set_profiling(True)
    samples = []
    for _ in range(5):
        run()
        torch.cuda.synchronize()
        samples.append(e.op_times())
    kern = e.op_kernels()
    e.set_profiling(False)
    ms = {k: statistics.median(s[k] for s in samples) for k in samples[0]}
    total = sum(ms.values())
    prog = {o['name']: o for o in arch.program()}
    lines = [f'# scripts/gpu_resenc_case.py: ResEnc-M-like 2-D net, features {feats}, blocks {blocks}, B = {B}, {H} x {W}, split mode, {torch.cuda.get_device_name(0)}',
             f'# median of 5 profiled forwards; sum of the launches {total:.3f} ms = {B / total * 1e3:.1f} slices/s; {arch.work(H, W)["flops"] * B / total / 1e9:.1f} TFLOP/s algorithmic',
             f'{"launch":<22} {"kernel":<24} {"ms":>8} {"share":>7}  note']
    fam = {'res_join': 0.0, 'pool_proj1x1': 0.0, 'pool_proj1x1 statistics': 0.0}
    for name, t in ms.items():
        op = prog.get(name)
        note = ''
        if op is not None and op['op'] == OP_JOIN:
            h, w = arch.extent(op['level'], H, W)
            win = op['stride'][0] * op['stride'][1]
            nbytes = B * h * w * op['cout'] * 4 * (2 + win)
            note = f'{nbytes / t / 1e9:.2f} TB/s of {HBM_COPY_TBS} (copy, profiles/r02_hbm_probe.txt)'
            fam['res_join'] += t
        elif op is not None and op['op'] == OP_PROJ1X1:
            h, w = arch.extent(op['level'], H, W)
            fl = 2.0 * B * h * w * op['cin'] * op['cout']
            note = f'{fl / t / 1e9:.1f} TFLOP/s of {F32_MFMA_TFS} (fp32 MFMA peak)'
            fam['pool_proj1x1'] += t
        elif name.endswith('.proj.stats'):
            fam['pool_proj1x1 statistics'] += t
        lines.append(f'{name:<22} {kern.get(name, ""):<24} {t:8.3f} {t / total:7.2%}  {note}')
    lines.append('# shares of the forward: ' + ', '.join(f'{k} {v:.3f} ms = {v / total:.2%}' for k, v in fam.items()))
    text = '\n'.join(lines) + '\n'
    print(text)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(text)
    e.close()


if __name__ == '__main__':
    main()
