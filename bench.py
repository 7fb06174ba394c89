#!/usr/bin/env python3
"""bench.py - BASELINE.json metric: 2-ch 512x512 slices/sec on N MI355X (config 2: synthetic batch=64, one ts2d-v2
sub-model (K=18), fp32).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: either under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...`, or plain
     `python bench.py --gpus N`: with no WORLD_SIZE in the environment the script starts that launcher itself as a CHILD process -
     one rank per GPU, the reference's counterpart being its `mp.Pool` of workers, ts2d/core/inference/predictor.py:79-86 -
     and relays rank 0's line and the exit code.  TS2D_BENCH_DRYRUN=gloo runs the N-rank control path on the CPU: process group,
     weight-blob broadcast, slice sharding, time reduction; no GPU call.)

One "step" = one forward pass of the hot path (the whole PlainConvUNet, input NCHW -> fp32 logits NCHW + packed masks)
over one batch of 64 synthetic slices per GPU, inputs already resident in HBM.  Slices shard over ranks with no
data-path collective (weak scaling); weights are broadcast once from rank 0 with RCCL before the timed region.
Rank 0 prints ONE JSON line.  The inputs come from a fixed seed, so the same arguments give the same batch in every run;
`--dump-outputs DIR` writes what the last timed step left in the caller's buffers (rank 0: DIR/logits.npy, DIR/mask.npy; see
dump_outputs), so that two builds of the library can be compared output for output.

A plain run does what the headline needs and no more: set-up, warm-up, the timed steps, the dump if asked for, the line.  The
per-kernel HIP events sampled inside the timed steps are part of the step definition, so the roofline blocks computed from them
come with every line at no cost.  `--full` adds what takes runs of its own, outside the timed region: the other precision modes
with their oracle errors and roofline blocks, the other extents (`geometry`), BASELINE configurations 3 and 5, the live oracle
check of the timed batch and the CPU baseline; on N > 1 GPUs also the config-4 stream as `stream_10k`.  `--no-cpu-baseline`,
`--no-other-modes` and `--no-extra-legs` take single legs out of a `--full` run again.

Other BASELINE configurations (same contract, ONE JSON line each; `config.workload` names the configuration):
    python bench.py --workload config3          five ts2d-v2 sub-models (117 labels) on one batch of 128, 16-bit mode
    python bench.py --workload config4 [--stream 10000]   (N ranks) contiguous blocks of a 10k-slice stream generated on the
                                                device from (seed, slice index); strong scaling; weight broadcast reported
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3     # v_mfma_f32_32x32x2_f32, 64 FLOP/clk/SIMD
PEAK_F16_MFMA_TFLOPS = 2500.0     # dense fp16/bf16 MFMA peak; the split path issues 3 fp16 MFMA products per MAC
MEASURED_F16_PIPE_TFLOPS = 32768 * 1024 / 20.8e-9 / 1e12      # 32x32x16 MFMA = 32768 FLOP, 1024 SIMDs, 20.8 ns each (probe): ~1613
PEAK_HBM_GBS = 8000.0
MEASURED_HBM_MIXED_GBS = 4700.0   # copy / 4:3 read:write streaming rate measured on this pool (scripts/probes/hbm_probe.hip)


def host_cores() -> int:
    """Threads for the CPU baseline: the process's CPU share (affinity mask, cgroup quota), capped at 16 - the
    per-GPU host share of the pool's boxes (a 256-thread pool on a 16-core share ran 30x slower)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()
        if quota != 'max':
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, min(n, int(os.environ.get('TS2D_CPU_THREADS', 16))))


def host_cpu_model() -> str:
    """Model name of the host CPU (the baseline wanders 3.9 ... 5.3 slices/s between boxes of the pool: this says why)."""
    try:
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.lower().startswith('model name'):
                    return line.split(':', 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine()


def cpu_baseline(arch, sd, budget_s: float = 20.0, check=None):
    """The oracle (torch-CPU restatement = the ATen kernels the reference CPU path runs), B = 1 per call like the
    reference, all host cores, on a bounded sample of the same workload.  `check` = (x, gpu logits)
    of one slice: the oracle's output on it gives the live logit max-abs-err of the metric."""
    import torch
    from oracle import torch_oracle as O
    cores = host_cores()
    torch.set_num_threads(cores)
    x = torch.randn(1, arch.input_channels, 512, 512)
    err = None
    if check is not None:
        ref = O.unet_forward(arch, sd, check[0]).numpy()         # doubles as the warm-up
        err = float(np.abs(ref - check[1]).max())
    else:
        O.unet_forward(arch, sd, x)                  # warm-up
    t0 = time.time()
    n = 0
    while n < 3 or (time.time() - t0 < budget_s and n < 64):
        O.unet_forward(arch, sd, x)
        n += 1
    dt = time.time() - t0
    return {'value': round(n / dt, 3), 'unit': 'slices/s', 'cores': cores, 'cpu_model': host_cpu_model(), 'kind': 'port',
            'sample': f'{n} single-slice (B=1, no mirroring) 2x512x512 forwards of the same network, torch-CPU oracle, '
                      f'{torch.get_num_threads()} threads'}, err


def csrc_hash() -> str:
    """Hash of the kernel sources: profiles/pmc_traffic.json is stamped with it so that a stale PMC figure is not reported
    against kernels it was not measured on."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
    for f in sorted(os.listdir(d)):
        if f.endswith(('.h', '.hip')):
            h.update(f.encode()); h.update(open(os.path.join(d, f), 'rb').read())
    return h.hexdigest()[:16]


SIGMOID_HALF_THRESHOLD = 1.5 * 2.0 ** -24       # sigmoid(float(x)) > 0.5  <=>  x > 1.5 * 2^-24 (tests/test_oracle.py pins it)


def oracle_check(arch, sd, x4, logits4, mask4, emulate=None):
    """Live parity of the metric's own outputs: `x4` slices of the timed batch through the torch-CPU oracle (`emulate='f16'`: the
    16-bit mode's own arithmetic contract).  Returns per-slice max-abs errors, the number of differing mask bits, the bits checked
    and, over the differing bits, the largest |oracle logit - threshold| together with whether every one of them lies within its
    slice's logit error of the threshold (i.e. is a tolerance flip, not a wrong mask)."""
    from oracle import torch_oracle as O
    from totalsegmentator2d_amd.engine import unpack_mask
    errs, flips, bits, worst, all_tol = [], 0, 0, 0.0, True
    for i in range(x4.shape[0]):
        ref = O.unet_forward(arch, sd, x4[i:i + 1], emulate=emulate).numpy()
        errs.append(float(np.abs(ref - logits4[i:i + 1]).max()))
        if mask4 is not None:
            m_ref = O.logits_to_mask(ref).numpy()
            m_gpu = unpack_mask(mask4[i:i + 1], x4.shape[-1])
            d = m_ref != m_gpu
            flips += int(d.sum()); bits += int(m_ref.size)
            if d.any():
                dist = float(np.abs(ref[d].astype(np.float64) - SIGMOID_HALF_THRESHOLD).max())
                worst = max(worst, dist)
                all_tol = all_tol and dist <= errs[-1]
    return errs, flips, bits, worst, all_tol


DUMP_ELEMS = 1 << 22              # --dump-outputs: elements kept per array (16 MB as float32, 32 MB for the two arrays)


def dump_outputs(torch, d, logits, mask):
    """`--dump-outputs d`: the two arrays a caller of the timed step receives, as d/logits.npy (fp32 logits) and d/mask.npy (the packed
    mask words unpacked to 0.0 / 1.0 per pixel, float32).  Arrays of more than DUMP_ELEMS elements are sampled: the same positions
    of both, DUMP_ELEMS flat indices into the B x K x H x W logits drawn from a fixed seed (sorted, repeats dropped) - every slice, label and
    image region is covered, and the files of two runs with the same arguments line up element for element."""
    n = logits.numel()
    if n > DUMP_ELEMS:
        idx = torch.from_numpy(np.unique(np.random.default_rng(0).integers(0, n, DUMP_ELEMS))).to(logits.device)
    else:
        idx = torch.arange(n, device=logits.device)
    # bit w % 32 of word w // 32 of a row is pixel w (engine.unpack_mask); W is a multiple of 32, so the same holds for flat indices
    bits = (mask.reshape(-1)[idx // 32] >> (idx % 32)) & 1
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, 'logits.npy'), logits.reshape(-1)[idx].cpu().numpy().astype(np.float32, copy=False))
    np.save(os.path.join(d, 'mask.npy'), bits.cpu().numpy().astype(np.float32))


def timed_forward(torch, dev, fn, rounds=3, reps=3):
    """Median over `rounds` of the mean device time of `reps` back-to-back calls (torch events on the current stream), ms."""
    fn(); fn()
    torch.cuda.synchronize(dev)
    ts = []
    st = torch.cuda.current_stream(dev)
    for _ in range(rounds):
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(st)
        for _ in range(reps):
            fn()
        t1.record(st)
        torch.cuda.synchronize(dev)
        ts.append(t0.elapsed_time(t1) / reps)
    return float(np.median(ts))


def geometry_leg(torch, dev, engine, arch, B, H, W, modes=('split', 'f16')):
    """Throughput and kernel dispatch of `engine` on a B x C x H x W batch (logits + packed masks out, inputs resident), per mode:
    slices/s, Mpixel/s and the kernel that served every op.  The reference runs whatever patch size / pooling plans.json names
    (ts2d/core/inference/prediction_worker.py:76-77, nnu.py:164-165); 512 x 512 is this repo's ASSUMPTION."""
    x = torch.randn(B, arch.input_channels, H, W, device=dev)
    lg = torch.empty(B, arch.num_classes, H, W, device=dev)
    mk = torch.empty(B, arch.num_classes, H, W // 32, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {'batch': B, 'H': H, 'W': W, 'n_stages': arch.n_stages, 'strides_last': list(arch.strides[-1]),
           'gflop_per_slice': round(arch.work(H, W)['flops'] / 1e9, 2)}
    for mode in modes:
        engine.set_precision(mode)
        engine.set_profiling(False)
        ms = timed_forward(torch, dev, lambda: engine.forward(x, logits=True, mask=True, out_logits=lg, out_mask=mk, stream=stream))
        engine.set_profiling(True)
        engine.forward(x, logits=True, mask=True, out_logits=lg, out_mask=mk, stream=stream)
        torch.cuda.synchronize(dev)
        kern = {k: v for k, v in engine.op_kernels().items() if not k.endswith('.stats')}
        engine.set_profiling(False)
        out[mode] = {'ms_per_step': round(ms, 3), 'slices_per_s': round(B / ms * 1e3, 1), 'mpixel_per_s': round(B * H * W / ms * 1e-3, 1),
                     'tflops': round(B / ms * 1e3 * arch.work(H, W)['flops'] / 1e12, 1), 'kernels': kern}
    del x, lg, mk
    return out


def config3_leg(torch, dev, local_rank, body_sd, B=128, steps=3):
    """BASELINE configs[2] inside the default line: the five ts2d-v2 sub-models (K = 18/23/24/26/26 -> 117 mask channels) on one batch of
    128 slices, one shared activation workspace, 16-bit mode, packed masks out.  (The reference drives its five sub-models per case
    one after the other: ts2d/tool.py:110-112.)  Throughput does not depend on the weight values: the four other sub-models reuse
    sub-model 1's body tensors with heads of their own (generating five 46 M-parameter sets costs 40 s of host time; `--workload
    config3` and the tests use five independent sets)."""
    from totalsegmentator2d_amd import parallel, weights
    from totalsegmentator2d_amd.arch import UNetArch
    from totalsegmentator2d_amd.submodels import SubModelSet, TS2D_V2_HEADS
    models = []
    for i, mid in enumerate(sorted(TS2D_V2_HEADS)):
        a = UNetArch.canonical(num_classes=TS2D_V2_HEADS[mid])
        sd = dict(body_sd)
        for t, (key, shp) in enumerate(a.param_specs()):
            if 'seg_layers' in key:
                sd[key] = weights.prng.normal_f32(i + 1, t, shp, mean=0.0, std=0.05 if key.endswith('weight') else 0.01)
        models.append((mid, a, weights.pack_blob(a, sd)))
    x = parallel.synth_slices(local_rank, 0, 0, B, (2, 512, 512))
    res = {'workload': 'BASELINE configs[2]: full ts2d-v2 (5 sub-models, 117 labels), batch=128, 1xMI355X, packed masks out', 'batch': B}
    with SubModelSet(models, device=local_rank, precision='f16') as ms:
        ms.reserve(B, 512, 512)
        stream = torch.cuda.current_stream(dev).cuda_stream
        masks = ms.forward_masks(x, stream=stream)
        work = sum(e.arch.work(512, 512)['flops'] for e in ms.engines)
        for mode in ('f16', 'split'):
            ms.set_precision(mode)
            t = timed_forward(torch, dev, lambda: ms.forward_masks(x, masks, stream=stream), rounds=steps, reps=1)
            res[mode] = {'ms_per_batch': round(t, 2), 'value': round(B / t * 1e3, 1), 'unit': 'slices/s (all five sub-models)',
                         'sub_model_forwards_per_s': round(5 * B / t * 1e3, 1), 'tflops': round(B / t * 1e3 * work / 1e12, 1)}
        res['labels'] = int(sum(ms.channels))
    del x, masks
    return res


def config5_leg(torch, dev, local_rank, B=32):
    """BASELINE configs[4] geometry on one GPU: tsxr X-ray path, 1 x 1024 x 1024, 9 stages, K = 26 (ribs: the reference's xr test model,
    ts2d/data/config.json:4), 16-bit and split modes, packed masks out: images/s, TFLOP/s and the stride-1 3x3 family's fraction of
    the MFMA peak (HIP events of one profiled forward)."""
    from totalsegmentator2d_amd import weights
    from totalsegmentator2d_amd.arch import UNetArch, OP_CONV3X3
    from totalsegmentator2d_amd.engine import Engine
    a = UNetArch.canonical(input_channels=1, num_classes=26, n_stages=9)
    w = a.work(1024, 1024)
    fam = {o['name']: 2.0 * m['macs'] for o, m in zip(a.program(), w['per_layer'])
           if o['op'] == OP_CONV3X3 and tuple(o['stride']) == (1, 1) and o['src'] != 'input'}
    res = {'workload': 'BASELINE configs[4] on one GPU: tsxr 1x1024x1024, 9 stages, K=26, packed masks out', 'batch': B,
           'gflop_per_image': round(w['flops'] / 1e9, 2)}
    with Engine(a, weights.pack_blob(a, weights.synthetic_state_dict(a, 7)), device=local_rank) as e:
        x = torch.randn(B, 1, 1024, 1024, device=dev)
        m = torch.empty(B, 26, 1024, 32, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for mode, peak in (('f16', PEAK_F16_MFMA_TFLOPS), ('split', PEAK_F16_MFMA_TFLOPS / 3.0)):
            e.set_precision(mode)
            t = timed_forward(torch, dev, lambda: e.forward(x, logits=False, mask=True, out_mask=m, stream=stream), rounds=3, reps=1)
            e.set_profiling(True)
            e.forward(x, logits=False, mask=True, out_mask=m, stream=stream)
            torch.cuda.synchronize(dev)
            ot = e.op_times()
            e.set_profiling(False)
            fms = sum(v for k, v in ot.items() if k in fam)
            ftf = sum(fam.values()) * B / (fms * 1e-3) / 1e12
            res[mode] = {'ms_per_batch': round(t, 2), 'value': round(B / t * 1e3, 1), 'unit': 'images/s', 'tflops': round(B / t * 1e3 * w['flops'] / 1e12, 1),
                         'stride1_family': {'ms': round(fms, 3), 'achieved_tflops': round(ftf, 1), 'peak': round(peak, 1), 'frac': round(ftf / peak, 4)}}
        del x, m
    return res


def run_config3(args, torch, dev, local_rank):
    """BASELINE config 3: full ts2d-v2 (5 sub-models, 117 labels), batch 128, one MI355X, 16-bit mode."""
    from totalsegmentator2d_amd import parallel, weights
    from totalsegmentator2d_amd.arch import UNetArch
    from totalsegmentator2d_amd.submodels import SubModelSet, TS2D_V2_HEADS
    B = 128 if args.batch == 64 else args.batch
    models = []
    for i, mid in enumerate(sorted(TS2D_V2_HEADS)):
        a = UNetArch.canonical(num_classes=TS2D_V2_HEADS[mid])
        models.append((mid, a, weights.pack_blob(a, weights.synthetic_state_dict(a, seed=i + 1))))
    x = parallel.synth_slices(local_rank, 0, 0, B, (2, 512, 512))
    with SubModelSet(models, device=local_rank, precision=args.precision) as ms:
        ms.reserve(B, 512, 512)
        stream = torch.cuda.current_stream(dev).cuda_stream
        masks = ms.forward_masks(x, stream=stream)
        for _ in range(max(args.warmup - 1, 0)):
            ms.forward_masks(x, masks, stream=stream)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ms.forward_masks(x, masks, stream=stream)
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        merged = SubModelSet.merge(masks)
        torch.cuda.synchronize(dev)
        work = sum(e.arch.work(512, 512)['flops'] for e in ms.engines)
        out = {'metric': '2-ch 512x512 slices/sec', 'value': round(B * args.steps / el, 2), 'unit': 'slices/s', 'n_gpus': 1,
               'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(el / args.steps * 1e3, 3), 'higher_is_better': True,
               'scaling': 'weak', 'vs_baseline': None,
               'dtype': {'f16': 'f16 storage + f16 MFMA, f32 accumulate/statistics', 'split': 'f32 storage, 3x fp16-split MFMA', 'exact': 'f32'}[args.precision],
               'data': 'synthetic',
               'config': {'workload': 'BASELINE configs[2]: full ts2d-v2 (5 sub-models, K = 18/23/24/26/26 -> 117 labels), batch=128, '
                                      '1xMI355X, 16-bit mode (fp16 storage; the config says bf16 - DESIGN.md section 4), packed masks out',
                          'batch_per_gpu': B, 'sub_models': ms.ids, 'labels': int(merged.shape[1]), 'H': 512, 'W': 512,
                          'gflop_per_slice_all_models': round(work / 1e9, 1)},
               'sub_model_forwards_per_s': round(5 * B * args.steps / el, 1), 'tflops': round(B * args.steps / el * work / 1e12, 1),
               'precision_mode': args.precision}
    print(json.dumps(out), flush=True)


def run_config4(args, torch, dev, engine, rank, world, total, seed=0, batch=64, reduce=True):
    """BASELINE config 4 on this rank: its contiguous block of the `total`-slice stream (generated on the device beforehand)."""
    from totalsegmentator2d_amd import parallel
    engine.set_precision(args.precision)
    werr = None
    try:
        parallel.run_slice_stream(engine, seed, min(total, 2 * batch * world), rank, world, batch=batch, keep_masks=False)   # warm-up
    except Exception as ex:                                                # noqa: BLE001
        werr = f'{type(ex).__name__}: {ex}'
    # the barrier in front of the timed region doubles as the agreement that every rank got through its warm-up: a rank that
    # failed still reaches it, and then ALL ranks raise (nobody is left waiting in a collective)
    if parallel.max_over_ranks(1.0 if werr else 0.0) > 0:
        raise RuntimeError(werr or 'config-4 warm-up failed on another rank')
    lo, hi, masks, dt = parallel.run_slice_stream(engine, seed, total, rank, world, batch=batch, keep_masks=True)
    el = parallel.max_over_ranks(dt) if reduce else dt            # reduce=False: the caller reduces (after agreeing that no rank failed)
    biggest = max(b - a for a, b in (parallel.shard_range(total, r, world) for r in range(world)))     # remainder ranks hold one more
    return {'slices': total, 'block_of_rank0': [lo, hi], 'seconds': round(el, 4), 'value': round(total / el, 2), 'unit': 'slices/s',
            'batch': batch, 'steps': (biggest + batch - 1) // batch, 'mask_words_kept': int(masks.numel()) if masks is not None else 0}


def free_port() -> int:
    import socket
    with socket.socket() as so:
        so.bind(('127.0.0.1', 0))
        return so.getsockname()[1]


def self_launch(n: int) -> int:
    """`python bench.py --gpus N` outside torchrun: start `torch.distributed.run` with N ranks of this script as a child
    process (never os.exec*: nothing here has touched the GPU, but the child is still the safe form), stdout / stderr inherited so
    rank 0's single JSON line goes straight through; returns the child's exit code."""
    import subprocess
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
           '--master-port', str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    env.setdefault('OMP_NUM_THREADS', str(max(1, host_cores() // n)))
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')            # dmabuf IPC: RCCL across processes needs it on this pool
    return subprocess.run(cmd, env=env).returncode


def dry_run(args, backend: str):
    """TS2D_BENCH_DRYRUN=<backend> (gloo): the multi-rank CONTROL path of this script without a GPU - process group, weight
    broadcast (the host blob instead of the device arena), the config-4 slice blocks, the barrier + max-over-ranks reduction of
    the timed region - on a narrow net; rank 0 prints one line with `n_gpus` = world."""
    import torch.distributed as dist
    from totalsegmentator2d_amd import parallel, weights
    from totalsegmentator2d_amd.arch import UNetArch
    rank, _, world = parallel.env_rank_world()
    parallel.init_process_group(backend)
    arch = UNetArch.canonical(input_channels=2, num_classes=2, n_stages=2, base=32, max_features=32)
    blob = weights.pack_blob(arch, weights.synthetic_state_dict(arch, seed=1)) if rank == 0 else None
    got = parallel.broadcast_blob(blob, arch.n_params(), src=0)
    lo, hi = parallel.shard_range(10000, rank, world)
    dist.barrier()
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))                                # "K steps": rank r takes r + 1 ticks, the max is reported
    dist.barrier()
    el = parallel.max_over_ranks(time.perf_counter() - t0)
    sizes = [0] * world
    import torch
    t = torch.zeros(world, dtype=torch.int64); t[rank] = hi - lo
    dist.all_reduce(t)
    sizes = [int(v) for v in t]
    if rank == 0:
        print(json.dumps({'metric': '2-ch 512x512 slices/sec', 'value': None, 'unit': 'slices/s', 'n_gpus': world, 'steps': args.steps,
                          'warmup': args.warmup, 'dry_run': backend, 'blob_floats': int(got.size), 'blob_sum': float(np.float64(got.sum())),
                          'stream_blocks': sizes, 'stream_steps': (max(sizes) + args.batch - 1) // args.batch,
                          'elapsed_max_s': round(el, 4)}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=64, help='slices per GPU per step (config 2: 64)')
    ap.add_argument('--full', action='store_true',
                    help='config 2: after the timed steps also run every leg the headline does not need (other precision modes, other extents, '
                         'configs 3 and 5, oracle check of the timed batch, CPU baseline; N > 1: the config-4 stream); off by default')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full without the oracle checks and the CPU baseline')
    ap.add_argument('--no-profile', action='store_true', help='do not bracket kernels with HIP events')
    ap.add_argument('--no-other-modes', action='store_true', help='--full without the exact / f16 legs (and without the legs of --no-extra-legs)')
    ap.add_argument('--no-extra-legs', action='store_true', help='--full without the geometry / config3 / config5 legs')
    ap.add_argument('--workload', choices=('config2', 'config3', 'config4'), default='config2')
    ap.add_argument('--stream', type=int, default=None, help='config 4: total slices of the synthetic stream (default 10000)')
    ap.add_argument('--precision', choices=('split', 'exact', 'f16'), default=None,
                    help="split: fp16 hi/lo x3 MFMA with fp32 accumulation (fp32-equivalent accuracy, default); exact: fp32 MFMA; "
                         "f16: fp16 storage + one fp16 MFMA product (BASELINE configs 3/5, outside the fp32 parity tolerance)")
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='config 2: after the timed steps rank 0 writes the logits and masks of the last one (a fixed sample) as DIR/<name>.npy')
    args = ap.parse_args(argv)
    if args.stream is not None and args.workload == 'config2':
        args.workload = 'config4'
    if args.precision is None:
        args.precision = 'f16' if args.workload == 'config3' else 'split'
    if args.dump_outputs is not None and (args.workload != 'config2' or os.environ.get('TS2D_BENCH_DRYRUN')):
        ap.error('--dump-outputs is implemented for the config-2 workload on a GPU only')
    if not args.full:                 # a plain run: no leg besides the timed steps
        args.no_cpu_baseline = args.no_other_modes = args.no_extra_legs = True
    return args


def main():
    args = parse_args()
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # not under a launcher: start one (child process), relay its exit code; nothing below runs in this process
        raise SystemExit(self_launch(args.gpus))
    if os.environ.get('TS2D_BENCH_DRYRUN'):
        dry_run(args, os.environ['TS2D_BENCH_DRYRUN'])
        return

    import torch
    import torch.distributed as dist
    from totalsegmentator2d_amd import parallel, weights
    from totalsegmentator2d_amd.arch import UNetArch, OP_CONV3X3
    from totalsegmentator2d_amd.engine import Engine

    rank, local_rank, world = parallel.env_rank_world()
    if world != args.gpus:
        if args.gpus > 1:
            raise SystemExit(f"--gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    multi = world > 1 or os.environ.get('TS2D_FORCE_DIST') == '1'      # the flag rehearses the RCCL path on one GPU
    if multi:
        parallel.init_process_group('nccl')
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)

    if args.workload == 'config3':
        if world != 1:
            raise SystemExit('config 3 is a one-GPU configuration')
        run_config3(args, torch, dev, local_rank)
        return

    arch = UNetArch.canonical(input_channels=2, num_classes=18)            # one ts2d-v2 sub-model (cardiac, K = 18)
    B, H, W = args.batch, 512, 512
    sd = None
    if rank == 0:
        sd = weights.synthetic_state_dict(arch, seed=1)                    # He-normal, BASELINE.md section 4
        engine = Engine(arch, weights.pack_blob(arch, sd), device=local_rank)
    else:
        engine = Engine(arch, None, device=local_rank)
    if os.environ.get('TS2D_FORCE_DIST') == '1' and world == 1:
        # rehearsal: a second, empty replica on the same GPU receives the arena by device copy after the (self) broadcast
        replica = Engine(arch, None, device=local_rank)
    bcast_ms = None
    if multi:
        dist.barrier()
        t0 = time.time()
        parallel.broadcast_engine_weights(engine, src=0)                   # one RCCL broadcast over xGMI
        bcast_ms = (time.time() - t0) * 1e3
        if os.environ.get('TS2D_FORCE_DIST') == '1' and world == 1:
            ps, ns = engine.weight_buffer(); pd, nd = replica.weight_buffer()
            torch.as_tensor(parallel._DevicePtrTensor(pd, nd), device=dev).copy_(torch.as_tensor(parallel._DevicePtrTensor(ps, ns), device=dev))
            torch.cuda.synchronize(dev); replica.weights_ready()
            xa = torch.randn(2, 2, 512, 512, device=dev)
            la, _ = engine.forward(xa); lb, _ = replica.forward(xa); torch.cuda.synchronize(dev)
            assert torch.equal(la, lb), 'replica filled through the broadcast hook differs'
            replica.close()
    ranks_seen = None
    if multi:
        # (rank, device index, PCI bus id) of every rank, gathered over the process group: a SCALE line shows that RCCL saw N ranks on N devices
        try:
            bus = torch.cuda.get_device_properties(local_rank)
            mine = [rank, local_rank, int(getattr(bus, 'pci_bus_id', -1)), int(getattr(bus, 'pci_device_id', -1)), int(getattr(bus, 'pci_domain_id', -1))]
        except Exception:                                                  # noqa: BLE001
            mine = [rank, local_rank, -1, -1, -1]
        t = torch.tensor(mine, dtype=torch.int64, device=dev)
        got = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(got, t)
        ranks_seen = [{'rank': int(g[0]), 'device': int(g[1]), 'pci': f'{int(g[4]):04x}:{int(g[2]):02x}:{int(g[3]):02x}' if int(g[2]) >= 0 else None} for g in got]
    if args.workload == 'config4':
        total = args.stream if args.stream is not None else 10000
        r4 = run_config4(args, torch, dev, engine, rank, world, total, batch=B)
        if rank == 0:
            work = arch.work(H, W)
            out = {'metric': '2-ch 512x512 slices/sec', 'value': r4['value'], 'unit': 'slices/s', 'n_gpus': world,
                   'steps': r4['steps'], 'warmup': 2, 'ms_per_step': round(r4['seconds'] / max(1, r4['steps']) * 1e3, 3),
                   'higher_is_better': True, 'scaling': 'strong', 'vs_baseline': None,
                   'dtype': 'f32 storage/accumulate, products as 3x fp16-split MFMA (f16x3)' if args.precision == 'split' else args.precision,
                   'data': 'synthetic',
                   'config': {'workload': f'BASELINE configs[3]: {world}xMI355X slice-batch sharding, synthetic {total}-slice stream generated on the '
                                          'device from (seed, slice index), contiguous blocks per rank, RCCL weight broadcast before the timed region, '
                                          'packed masks of the whole stream kept', 'stream_slices': total, 'batch_per_step': B,
                              'parallelism': f'slice-dp{world}', 'gflop_per_slice': round(work['flops'] / 1e9, 2)},
                   'weight_broadcast_ms': None if bcast_ms is None else round(bcast_ms, 2), 'precision_mode': args.precision,
                   'tflops': round(r4['value'] * work['flops'] / 1e12, 2), 'ranks_seen': ranks_seen}
            print(json.dumps(out), flush=True)
        engine.close()
        if multi:
            dist.barrier()
            dist.destroy_process_group()
        return

    gen = torch.Generator(device=dev).manual_seed(1000 + rank)
    x = torch.randn(B, 2, H, W, device=dev, generator=gen)                 # synthetic N(0,1) = post-z-score statistics
    logits = torch.empty(B, arch.num_classes, H, W, device=dev)
    mask = torch.empty(B, arch.num_classes, H, W // 32, dtype=torch.int32, device=dev)
    engine.reserve(B, H, W)
    engine.set_precision(args.precision)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def step():
        engine.forward(x, logits=True, mask=True, out_logits=logits, out_mask=mask, stream=stream)

    for _ in range(args.warmup):
        step()
    profile = not args.no_profile and rank == 0
    # per-kernel HIP events bracket every launch of every THIRD timed step (steps 0, 3, 6, ...): the event pairs and the read-back
    # synchronisation cost 0.7 ms per profiled step (measured: 24.08 vs 24.77 ms/step), so sampling keeps `value` within 1 % of the
    # un-instrumented rate while the per-kernel durations still come from the timed region itself
    prof_every, n_prof = 3, 0
    op_ms, op_kernels = {}, {}
    torch.cuda.synchronize(dev)
    if multi:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(args.steps):
        sample = profile and i % prof_every == 0
        if profile:
            engine.set_profiling(sample)
        step()
        if sample:                                                         # HIP events on the launch stream, read per profiled step
            for k, v in engine.op_times().items():
                op_ms[k] = op_ms.get(k, 0.0) + v
            op_kernels = engine.op_kernels()
            n_prof += 1
    torch.cuda.synchronize(dev)
    if multi:
        dist.barrier()
    torch.cuda.synchronize(dev)
    elapsed = parallel.max_over_ranks(time.perf_counter() - t0)
    if args.dump_outputs is not None and rank == 0:                        # before the legs below run other modes into the same buffers
        dump_outputs(torch, args.dump_outputs, logits, mask)

    stream_res = None
    if world > 1 and args.full:            # config 4 on the same ranks (outside the timed region above): 10k-slice stream, contiguous blocks
        if profile:
            engine.set_profiling(False)
        # Isolated from the primary result: a failure on ANY rank is agreed on by all ranks (one max-reduce of a flag, so no rank
        # waits in a collective the failed one never reaches) and reported as stream_10k.error; the config-2 line is printed either way.
        err = None
        try:
            stream_res = run_config4(args, torch, dev, engine, rank, world, 10000, batch=B, reduce=False)
        except Exception as ex:                                            # noqa: BLE001 - reported, not hidden
            err = f'{type(ex).__name__}: {ex}'
        failed = parallel.max_over_ranks(1.0 if err else 0.0) > 0
        if failed:
            stream_res = {'error': err or 'failed on another rank'}
        else:
            el4 = parallel.max_over_ranks(stream_res['seconds'])
            stream_res.update(seconds=round(el4, 4), value=round(10000 / el4, 2))

    if rank == 0:
        work = arch.work(H, W)
        ms_per_step = elapsed / args.steps * 1e3
        value = world * B * args.steps / elapsed
        out = {
            'metric': '2-ch 512x512 slices/sec', 'value': round(value, 2), 'unit': 'slices/s', 'n_gpus': world,
            'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(ms_per_step, 3), 'higher_is_better': True,
            'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': 'BASELINE configs[1]: synthetic batch=64 2x512x512, one ts2d-v2 sub-model '
                                   '(canonical 8-stage PlainConvUNet, K=18), fp32, logits + packed masks out',
                       'batch_per_gpu': B, 'global_batch': world * B, 'H': H, 'W': W, 'K': arch.num_classes,
                       'parallelism': f'slice-dp{world}', 'gflop_per_slice': round(work['flops'] / 1e9, 2),
                       'act_mb_per_slice': round(work['act_bytes'] / 1e6, 1)},
            'tflops': round(value * work['flops'] / 1e12, 2),
        }
        if bcast_ms is not None:
            out['weight_broadcast_ms'] = round(bcast_ms, 2)
        if ranks_seen is not None:
            out['ranks_seen'] = ranks_seen
        if stream_res is not None:
            out['stream_10k'] = dict(stream_res, workload='BASELINE configs[3]: 10k-slice stream, contiguous blocks per rank (strong scaling)')
        split = args.precision == 'split'
        out['dtype'] = {'split': 'f32 storage/accumulate, products as 3x fp16-split MFMA (f16x3)', 'exact': 'f32',
                        'f16': 'f16 storage + f16 MFMA, f32 accumulate/statistics (NOT within the fp32 parity tolerance)'}[args.precision]
        out['precision_mode'] = args.precision
        if profile and op_ms:
            prog = arch.program()
            layer = {o['name']: (o, m) for o, m in zip(prog, work['per_layer'])}
            ms = {k: v / n_prof for k, v in op_ms.items()}
            # (a) the stride-1 3x3 family of round 1 (22 launches/step, 83 % of the FLOPs), kept for continuity
            per = {n: 2.0 * m['macs'] for n, (o, m) in layer.items() if o['op'] == OP_CONV3X3 and tuple(o['stride']) == (1, 1) and o['src'] != 'input'}
            conv_ms = sum(ms[k] for k in per if k in ms)
            conv_flops = sum(per.values()) * B
            peak = {'split': PEAK_F16_MFMA_TFLOPS / 3.0, 'exact': PEAK_FP32_MFMA_TFLOPS, 'f16': PEAK_F16_MFMA_TFLOPS}[args.precision]
            # (b) the DOMINANT KERNEL, chosen by measured time: ops grouped by the kernel that served them (ts2d_engine_op_kernel).
            #     Algorithmic FLOPs of an op = the reference's own arithmetic (2 x MACs of the conv; a composed block
            #     conv3x3_upc / _upq / _up0 also carries the MACs of the ConvTranspose2d it absorbed, whose own launch no longer exists).
            alg = {n: 2.0 * m['macs'] for n, (o, m) in layer.items()}
            COMPOSED = ('conv3x3_upc', 'conv3x3_upq', 'conv3x3_up0')     # kernels that absorbed the ConvTranspose2d in front of them
            groups = {}
            for n, kname in op_kernels.items():
                if n.endswith('.stats') or n not in ms or n not in alg:
                    continue
                g = groups.setdefault(kname, {'ops': [], 'ms': 0.0, 'flops': 0.0})
                g['ops'].append(n); g['ms'] += ms[n]; g['flops'] += alg[n] * B
                if kname.startswith(COMPOSED):
                    g['flops'] += alg.get(n.replace('.c0', '.up'), 0.0) * B
            pmc_avg, traffic_stale = {}, None
            pmc = os.path.join(ROOT, 'profiles', 'pmc_traffic.json')
            if os.path.exists(pmc):
                try:
                    pj = json.load(open(pmc))
                    traffic_stale = pj.get('csrc_hash') != csrc_hash()          # measured on other kernel sources: do not report it
                    pmc_avg = {} if (traffic_stale or args.precision != 'split') else pj.get('hbm_bytes_per_launch_avg', {})      # (counters were collected in split mode)
                except Exception:
                    pmc_avg = {}
            pipe = MEASURED_F16_PIPE_TFLOPS / (3.0 if split else 1.0)
            table = []
            for kname, g in sorted(groups.items(), key=lambda kv: -kv[1]['ms']):
                tf = g['flops'] / (g['ms'] * 1e-3) / 1e12
                table.append({'kernel': kname, 'launches_per_step': len(g['ops']), 'ms_per_step': round(g['ms'], 3),
                              'share_of_step': round(g['ms'] / ms_per_step, 4), 'algorithmic_tflops': round(tf, 2),
                              'frac_of_peak': round(tf / peak, 4), 'hbm_bytes_per_launch': pmc_avg.get(kname), 'ops': sorted(g['ops'])})
            dom_kernel, dg = max(groups.items(), key=lambda kv: kv[1]['ms'])
            dom, dom_ms, dom_flops = dg['ops'], dg['ms'], dg['flops']
            achieved = dom_flops / (dom_ms * 1e-3) / 1e12
            traffic = pmc_avg.get(dom_kernel)
            all3 = {o['name'] for o in prog if o['op'] == OP_CONV3X3}
            out['roofline'] = {'bound': 'mfma', 'achieved': round(achieved, 2), 'peak': round(peak, 1), 'unit': 'TFLOP/s',
                               'frac': round(achieved / peak, 4), 'traffic': traffic, 'traffic_stale': traffic_stale,
                               'kernel': f'{dom_kernel} ({len(dom)} launches/step: {", ".join(sorted(dom))})',
                               'peak_note': ('dense fp16 MFMA 2500 TFLOP/s / 3 products per MAC' if split else
                                             ('dense fp16 MFMA' if args.precision == 'f16' else 'fp32 MFMA 32x32x2')),
                               # scripts/probes/mfma_shape_probe.hip: v_mfma_f32_32x32x16_f16 on every SIMD, operands from registers, random data
                               'frac_of_measured_matrix_pipe_rate': round(achieved / pipe, 4) if args.precision in ('split', 'f16') else None,
                               'algorithmic_flop_per_launch_avg': round(dom_flops / len(dom)),
                               'kernel_ms_per_launch_avg': round(dom_ms / len(dom), 4),
                               'kernel_ms_per_step': round(dom_ms, 3), 'kernel_share_of_step': round(dom_ms / ms_per_step, 4)}
            out['roofline_kernels'] = table
            fam = conv_flops / (conv_ms * 1e-3) / 1e12
            out['roofline_stride1_family'] = {'bound': 'mfma', 'achieved': round(fam, 2), 'peak': round(peak, 1), 'unit': 'TFLOP/s',
                                              'frac': round(fam / peak, 4), 'launches_per_step': len(per), 'ms_per_step': round(conv_ms, 3),
                                              'note': 'all 22 stride-1 3x3 launches (round-1 definition); its level-0 members are HBM-bound, see roofline_level0',
                                              'all_conv3x3_ms_per_step': round(sum(ms[k] for k in all3 if k in ms), 3)}
            # (c) level 0 + head: HBM-bound.  Algorithmic bytes = one read of every input (no halo), one write of the output.
            esz = 2 if args.precision == 'f16' else 4
            l0, l0_moved = {}, {}
            # with the first block fused into the second (conv3x3_first_stats + conv3x3_res32f) enc0.c0's output is never written and never
            # read: the MOVED bytes leave both out (the statistics pass and the fused block each read the network input instead)
            fused0 = op_kernels.get('enc0.c0') == 'conv3x3_first_stats'
            for n, (o, m) in layer.items():
                if o['level'] == 0 and n in ms:
                    cin = o['cin'] + o.get('cin_skip', 0)
                    px_in = (H * W) if o['op'] != 1 else (H * W) // 4          # transposed conv reads the level below
                    rd = px_in * cin * (4 if o['src'] == 'input' else esz)
                    if op_kernels.get(n, '').startswith(COMPOSED):           # composed block: reads the COARSE tensor instead of `up`
                        rd = ((H * W) // 4 * layer[n.replace('.c0', '.up')][0]['cin'] + H * W * o['cin_skip']) * esz
                    wr = H * W * o['cout'] * (4 if n == 'head' else esz)
                    l0[n] = (rd + wr) * B
                    mrd, mwr = rd, wr
                    if fused0 and n == 'enc0.c0':
                        mwr = 0
                    if fused0 and n == 'enc0.c1':
                        mrd = H * W * arch.input_channels * 4
                    l0_moved[n] = (mrd + mwr) * B
            l0_ms = sum(ms[k] for k in l0)
            l0_gbs = sum(l0.values()) / (l0_ms * 1e-3) / 1e9
            l0_mgbs = sum(l0_moved.values()) / (l0_ms * 1e-3) / 1e9
            out['roofline_level0'] = {'bound': 'hbm', 'achieved': round(l0_gbs, 1), 'peak': PEAK_HBM_GBS, 'unit': 'GB/s',
                                      'frac': round(l0_gbs / PEAK_HBM_GBS, 4), 'ops': sorted(l0), 'ms_per_step': round(l0_ms, 3),
                                      'moved': {'achieved': round(l0_mgbs, 1), 'frac': round(l0_mgbs / PEAK_HBM_GBS, 4), 'first_block_fused': fused0,
                                                'gb_per_step': round(sum(l0_moved.values()) / 1e9, 2), 'algorithmic_gb_per_step': round(sum(l0.values()) / 1e9, 2),
                                                'note': 'bytes the kernels actually move: enc0.c0 output neither written nor read when the first block is '
                                                        'recomputed inside the second; `achieved` above charges the layer-wise (reference) bytes'},
                                      'frac_of_measured_mixed_read_write_rate': round(l0_gbs / MEASURED_HBM_MIXED_GBS, 4),
                                      'note': 'scripts/probes/hbm_probe.hip on this pool: read-only 6.47, write-only 5.6, copy 4.7, 4:3 read:write '
                                              '4.6 TB/s; the achieved figure counts algorithmic bytes (halo re-reads not included)'}
            out['whole_step'] = {'hbm_frac_layerwise': round(value / world * work['act_bytes'] / 1e9 / PEAK_HBM_GBS, 4),
                                 'fp32_mfma_equiv_frac': round(value / world * work['flops'] / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4)}
            top = sorted(op_ms.items(), key=lambda kv: -kv[1])[:8]
            out['top_ops_ms'] = {k: round(v / n_prof, 3) for k, v in top}
            out['profiled_steps'] = n_prof
        if world == 1 and not args.no_other_modes:
            # the other arithmetic mode on the same workload (outside the timed region above; same step definition)
            other = 'exact' if split else 'split'
            out['f16_mode'] = None
            engine.set_profiling(False)
            engine.set_precision(other)
            step(); torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for _ in range(max(2, args.steps // 2)):
                step()
            torch.cuda.synchronize(dev)
            out['other_mode'] = {'precision_mode': other, 'value': round(B * max(2, args.steps // 2) / (time.perf_counter() - t1), 2), 'unit': 'slices/s'}
            if not args.no_cpu_baseline:                                # its own live error: slice 0 of the same batch through the oracle
                e1, *_ = oracle_check(arch, sd, x[:1].cpu().numpy(), logits[:1].cpu().numpy(), None)
                out['other_mode']['logit_max_abs_err_vs_oracle'] = {'value': e1[0], 'tol': 1e-4, 'slices_checked': 1}
            if profile and other == 'exact':
                # the strict-fp32 number (v_mfma_f32_32x32x2_f32: bit-for-bit an fp32 FMA chain) with its own roofline block
                engine.set_profiling(True)
                step(); torch.cuda.synchronize(dev)
                ot = engine.op_times()
                engine.set_profiling(False)
                ems = sum(v for k, v in ot.items() if k in per)
                each = conv_flops / (ems * 1e-3) / 1e12
                out['other_mode']['roofline'] = {'bound': 'mfma', 'achieved': round(each, 2), 'peak': PEAK_FP32_MFMA_TFLOPS, 'unit': 'TFLOP/s',
                                                 'frac': round(each / PEAK_FP32_MFMA_TFLOPS, 4), 'traffic': None,
                                                 'kernel': f'conv_mfma_f32<9,1,16,*> ({len(per)} launches/step)', 'kernel_ms_per_step': round(ems, 3)}
            if split:                                                   # third mode, for the record (configs 3/5 arithmetic)
                engine.set_precision('f16')
                step(); torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                for _ in range(max(2, args.steps // 2)):
                    step()
                torch.cuda.synchronize(dev)
                out['f16_mode'] = {'precision_mode': 'f16', 'value': round(B * max(2, args.steps // 2) / (time.perf_counter() - t1), 2), 'unit': 'slices/s',
                                   'note': 'fp16 storage + single fp16 MFMA product; logit rms error ~8e-3 vs the fp32 oracle, outside the 1e-4 parity tolerance'}
                if not args.no_cpu_baseline:
                    # live error against the 16-BIT oracle (the mode's own contract: fp16 weights / stored activations, fp32 accumulate)
                    # and against the fp32 oracle (what the mode costs), slice 0 of the timed batch
                    x1, l1, m1 = x[:1].cpu().numpy(), logits[:1].cpu().numpy(), mask[:1].cpu().numpy()
                    e16, fl16, b16, w16_, tol16 = oracle_check(arch, sd, x1, l1, m1, emulate='f16')
                    e32, *_ = oracle_check(arch, sd, x1, l1, None)
                    out['f16_mode']['logit_max_abs_err_vs_f16_oracle'] = {'value': e16[0], 'tol': 0.1, 'slices_checked': 1,
                                                                         'mask_bits_differing': fl16, 'mask_bits_checked': b16,
                                                                         'flips_all_within_logit_error_of_threshold': tol16}
                    out['f16_mode']['logit_max_abs_err_vs_fp32_oracle'] = e32[0]
                if profile:
                    # its own roofline block: the stride-1 3x3 family against the dense fp16 MFMA peak, and the whole step
                    # against HBM on the layer-wise activation bytes of 2-byte storage (arch.work(act_bytes=2))
                    engine.set_profiling(True)
                    step(); torch.cuda.synchronize(dev)
                    ot = engine.op_times()
                    engine.set_profiling(False)
                    hms = sum(v for k, v in ot.items() if k in per)
                    htf = conv_flops / (hms * 1e-3) / 1e12
                    w16 = arch.work(H, W, act_bytes=2)
                    hv = out['f16_mode']['value']
                    out['f16_mode']['roofline'] = {
                        'bound': 'mfma', 'achieved': round(htf, 2), 'peak': PEAK_F16_MFMA_TFLOPS, 'unit': 'TFLOP/s',
                        'frac': round(htf / PEAK_F16_MFMA_TFLOPS, 4), 'traffic': None,
                        'frac_of_measured_matrix_pipe_rate': round(htf / MEASURED_F16_PIPE_TFLOPS, 4),
                        'kernel': f'conv3x3_h2 / conv3x3_h32 / conv3x3_upc_h2 / conv3x3_up0 / conv3x3_res32 ({len(per)} stride-1 3x3 launches/step)',
                        'kernel_ms_per_step': round(hms, 3), 'step_ms_profiled': round(sum(ot.values()), 3),
                        'whole_step_tflops': round(hv * work['flops'] / 1e12, 1),
                        'whole_step_hbm': {'bound': 'hbm', 'achieved': round(hv * w16['act_bytes'] / 1e9, 1), 'peak': PEAK_HBM_GBS, 'unit': 'GB/s',
                                           'frac': round(hv * w16['act_bytes'] / 1e9 / PEAK_HBM_GBS, 4),
                                           'act_mb_per_slice': round(w16['act_bytes'] / 1e6, 1)}}
            engine.set_precision(args.precision)
        if world == 1 and not args.no_other_modes and not args.no_extra_legs:
            # ---- other extents and BASELINE configurations, outside the timed region (VERDICT r4 next #1c / #2)
            del logits, mask
            ref_mp = {'split': None, 'f16': None}
            geo = {'note': 'same engine / step definition as the headline (logits + packed masks out, inputs resident, B per GPU as given); '
                           'mpixel_per_s = B H W / time; ratio_to_512 = Mpixel/s relative to the 512 x 512 figure of the same mode in this block'}
            try:
                g512 = geometry_leg(torch, dev, engine, arch, B, 512, 512)
                for mode in ref_mp:
                    ref_mp[mode] = g512[mode]['mpixel_per_s']
                    g512[mode].pop('kernels')
                geo['512x512'] = g512
                g = geometry_leg(torch, dev, engine, arch, B, 640, 384)
                geo['640x384'] = g
                a7 = UNetArch.canonical(input_channels=2, num_classes=18, n_stages=7)
                with Engine(a7, weights.pack_blob(a7, weights.synthetic_state_dict(a7, seed=1)), device=local_rank) as e7:
                    geo['448x576_7stages'] = geometry_leg(torch, dev, e7, a7, B, 448, 576)
                for k in ('640x384', '448x576_7stages'):
                    for mode in ref_mp:
                        geo[k][mode]['ratio_to_512'] = round(geo[k][mode]['mpixel_per_s'] / ref_mp[mode], 4)
            except Exception as ex:                                        # noqa: BLE001 - reported, the headline is printed either way
                geo['error'] = f'{type(ex).__name__}: {ex}'
            out['geometry'] = geo
            engine.set_precision(args.precision)
            engine.reserve(B, H, W)
            for name, leg in (('config3', lambda: config3_leg(torch, dev, local_rank, sd)), ('config5', lambda: config5_leg(torch, dev, local_rank))):
                try:
                    out[name] = leg()
                except Exception as ex:                                    # noqa: BLE001
                    out[name] = {'error': f'{type(ex).__name__}: {ex}'}
            logits = torch.empty(B, arch.num_classes, H, W, device=dev)
            mask = torch.empty(B, arch.num_classes, H, W // 32, dtype=torch.int32, device=dev)
        if world == 1 and not args.no_cpu_baseline:
            step(); torch.cuda.synchronize(dev)
            idx = [0, B // 3, (2 * B) // 3, B - 1] if B >= 4 else list(range(B))
            import torch as _t
            sel = _t.tensor(idx, device=dev)
            errs, flips, bits, worst, all_tol = oracle_check(arch, sd, x[sel].cpu().numpy(), logits[sel].cpu().numpy(), mask[sel].cpu().numpy())
            out['cpu_baseline'], _ = cpu_baseline(arch, sd)
            out['logit_max_abs_err_vs_oracle'] = {'value': max(errs), 'per_slice': [round(e, 8) for e in errs], 'tol': 1e-4,
                                                  'slices_checked': len(idx), 'slice_indices': idx,
                                                  'note': 'outputs of the timed batch vs the torch-CPU oracle; full parity: pytest -m gpu'}
            # masks are bit-exact as a function of the engine's OWN logits (tests); against the oracle end to end a pixel whose
            # |logit| is below the logit error can fall on the other side of the threshold - reported, not hidden
            out['mask_disagree_vs_oracle'] = {'bits_differing': flips, 'bits_checked': bits, 'fraction': flips / max(bits, 1),
                                              'slices_checked': len(idx), 'max_abs_oracle_logit_at_flips': worst,
                                              'flips_all_within_logit_error_of_threshold': all_tol}
        print(json.dumps(out), flush=True)
    engine.close()
    if multi:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
