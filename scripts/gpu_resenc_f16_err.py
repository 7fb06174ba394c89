"""What the 16-bit mode of a ResidualEncoderUNet measures against its restatement (tests/resenc_f16_util.py) on one MI355X: every case of
tests/resenc_util.RES_CASES under both dispatches, per op on the engine's own inputs (the figures tests/test_gpu_resenc_f16.py asserts) and
end to end.  Measures only; the bounds are printed beside the maxima.

    python scripts/gpu_resenc_f16_err.py [profiles/r24_resenc_f16_err.txt]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import resenc_util as R                              # noqa: E402
from tests import test_gpu_resenc_f16 as T                      # noqa: E402
from tests import test_gpu_parity as P                          # noqa: E402
from tests import layer_check as LC                             # noqa: E402
from tests.conftest import blob_for                             # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    import torch
    lines = [f'# scripts/gpu_resenc_f16_err.py: 16-bit mode of the residual encoder against tests/resenc_f16_util.py, {torch.cuda.get_device_name(0)}',
             f'# bounds: per layer max {P.F16_LAYER_MAX} rms {P.F16_LAYER_RMS} (decoder entry rms {P.F16_LAYER_RMS_COMPOSED}), transposed conv {LC.F16_UP_RTOL} / head '
             f'{LC.HEAD_RTOL["f16"]} relative, join 1 of its bound and {T.JOIN_DIFFER_CAP} differing; end to end max {P.F16E_MAX} rms {P.F16E_RMS}, against float32 '
             f'max {P.F16_MAX} rms {P.F16_RMS}']
    worst = {}
    for name, (arch, B, H, W, seed) in R.RES_CASES.items():
        sd = blob_for(arch, seed)[0]
        x = R.case_input(name)
        for sbk in (0, 1):
            with T._engine(name, options={'sbk': sbk}) as e:
                e.set_profiling(True)
                e.keep_activations(True)
                lg = e.forward(x)[0]
                _, fig = T.check_ops(e, arch, sd, x, lg, f'{name} sbk={sbk}', check=False)
            d, d32 = lg - T.ref_logits(name), lg - R.oracle_logits(name)[0]
            fig.update({'logits vs the restatement, max': float(np.abs(d).max()), 'logits vs the restatement, rms': float(np.sqrt((d ** 2).mean())),
                        'logits vs float32, max': float(np.abs(d32).max()), 'logits vs float32, rms': float(np.sqrt((d32 ** 2).mean()))})
            lines.append(f'{name:<12} sbk={sbk}: ' + ', '.join(f'{k} {v:.3e}' for k, v in sorted(fig.items())))
            for k, v in fig.items():
                if v > worst.get(k, (-1.0,))[0]:
                    worst[k] = (v, f'{name} sbk={sbk}')
    lines.append('# worst over all cases and both dispatches:')
    lines += [f'#   {k:<44} {v:.3e}  ({where})' for k, (v, where) in sorted(worst.items())]
    text = '\n'.join(lines) + '\n'
    print(text)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
