"""ResidualEncoderUNet without a GPU: the plan -> descriptor mapping and its blob order, the restatement of the network against a module
tree with upstream's attribute names, the C-ABI entry and its binding, the model-folder loader, and the variants that are refused."""
import ctypes
import re

import numpy as np
import pytest

from tests import resenc_util as R
from tests.host_predictor import HostLogicPredictor
from totalsegmentator2d_amd import _lib, weights
from totalsegmentator2d_amd.arch import UNetArch

torch = pytest.importorskip('torch')


def _c3(key, co, ci):
    return [(f'{key}.conv.weight', (co, ci, 3, 3)), (f'{key}.conv.bias', (co,)), (f'{key}.norm.weight', (co,)), (f'{key}.norm.bias', (co,))]


# res_pool: features (32, 64, 64), blocks (1, 2, 2), 2 input channels, 5 classes, two convs per decoder stage - written out by hand
RES_POOL_SPECS = (
    _c3('encoder.stem.convs.0', 32, 2)
    + _c3('encoder.stages.0.blocks.0.conv1', 32, 32) + _c3('encoder.stages.0.blocks.0.conv2', 32, 32)
    + _c3('encoder.stages.1.blocks.0.conv1', 64, 32) + _c3('encoder.stages.1.blocks.0.conv2', 64, 64)
    + [('encoder.stages.1.blocks.0.skip.1.conv.weight', (64, 32, 1, 1)), ('encoder.stages.1.blocks.0.skip.1.norm.weight', (64,)),
       ('encoder.stages.1.blocks.0.skip.1.norm.bias', (64,))]
    + _c3('encoder.stages.1.blocks.1.conv1', 64, 64) + _c3('encoder.stages.1.blocks.1.conv2', 64, 64)
    + _c3('encoder.stages.2.blocks.0.conv1', 64, 64) + _c3('encoder.stages.2.blocks.0.conv2', 64, 64)          # (pool-only skip: no parameters)
    + _c3('encoder.stages.2.blocks.1.conv1', 64, 64) + _c3('encoder.stages.2.blocks.1.conv2', 64, 64)
    + [('decoder.transpconvs.0.weight', (64, 64, 2, 2)), ('decoder.transpconvs.0.bias', (64,))]
    + _c3('decoder.stages.0.convs.0', 64, 128) + _c3('decoder.stages.0.convs.1', 64, 64)
    + [('decoder.transpconvs.1.weight', (64, 32, 2, 2)), ('decoder.transpconvs.1.bias', (32,))]
    + _c3('decoder.stages.1.convs.0', 32, 64) + _c3('decoder.stages.1.convs.1', 32, 32)
    + [('decoder.seg_layers.1.weight', (5, 32, 1, 1)), ('decoder.seg_layers.1.bias', (5,))])


def test_from_plans_reads_a_resenc_plan_and_the_blob_order_is_the_hand_written_one():
    arch = R.RES_CASES['res_pool'][0]
    got = UNetArch.from_plans(R.plans_for(arch), '2d', 2, 5)
    assert got.encoder == 'residual' and tuple(got.n_blocks_per_stage) == (1, 2, 2)
    assert got == arch
    assert got.param_specs() == RES_POOL_SPECS
    names = [o['name'] for o in got.program()]
    assert names[:4] == ['stem', 'enc0.b0.c1', 'enc0.b0.c2', 'enc0.b0'] and 'enc1.b0.proj' in names and 'enc2.b0.proj' not in names
    prog = {o['name']: o for o in got.program()}
    assert prog['enc0.b0']['res'] == 'stem' and prog['enc1.b0']['res'] == 'enc1.b0.proj' and prog['enc1.b0']['stride'] == (1, 1)
    assert prog['enc2.b0']['res'] == 'enc1.b1' and prog['enc2.b0']['stride'] == (2, 2) and prog['enc1.b0.proj']['stride'] == (2, 2)
    assert prog['dec1.c0']['skip'] == 'enc1.b1' and prog['dec1.up']['src'] == 'enc2.b1'
    # the defaults are the plain net's: nothing that was constructed before changes
    plain = UNetArch.canonical()
    assert plain.encoder == 'plain' and tuple(plain.n_blocks_per_stage) == () and [o['name'] for o in plain.program()][:2] == ['enc0.c0', 'enc0.c1']
    d = got.to_dict()
    assert d['encoder'] == 'residual' and d['n_blocks_per_stage'] == [1, 2, 2]
    w = got.work(32, 48)
    assert len(w['per_layer']) == len(got.program()) and w['macs'] > 0


@pytest.mark.parametrize('name', list(R.RES_CASES))
def test_the_restatement_equals_a_module_tree_with_upstream_names(name):
    arch, B, H, W, seed = R.RES_CASES[name]
    sd = weights.synthetic_state_dict(arch, seed)
    net = R.build_replica(arch)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    assert sorted(net.state_dict()) == sorted(k for k, _ in arch.param_specs())
    x = R.case_input(name)
    with torch.no_grad():
        y_mod = net(torch.from_numpy(x)).numpy()
    y_fun = R.resenc_forward(arch, sd, x).numpy()
    assert y_mod.shape == (B, arch.num_classes, H, W) and y_mod.dtype == np.float32
    assert np.array_equal(y_mod, y_fun)


def test_the_residual_entry_is_declared_exported_and_bound():
    src = open(_lib.HEADER_PATH).read()
    body = re.search(r'typedef struct \{([^}]*)\} ts2d_residual_desc;', src, re.S)
    assert body, 'ts2d_residual_desc is not declared in include/ts2d_engine.h'
    decls = [' '.join(d.split()) for d in re.sub(r'/\*.*?\*/', '', body.group(1), flags=re.S).split(';') if d.strip()]
    assert decls == ['int32_t n_blocks[TS2D_MAX_STAGES]', 'int32_t reserved[16]']
    assert [f[0] for f in _lib.ResidualDesc._fields_] == ['n_blocks', 'reserved']
    assert ctypes.sizeof(_lib.ResidualDesc) == 4 * 32
    assert ctypes.sizeof(_lib.ArchDesc) == 4 * (3 + 3 * 16 + 2 + 2 * 16)                 # unchanged
    m = re.search(r'int\s+ts2d_engine_create_residual\s*\(([^)]*)\)\s*;', src)
    assert m, 'ts2d_engine_create_residual is not declared in include/ts2d_engine.h'
    assert [' '.join(p.split()) for p in m.group(1).split(',')] == ['const ts2d_arch_desc* arch', 'const ts2d_residual_desc* residual',
                                                                    'const float* weights', 'size_t n_floats', 'int device', 'ts2d_engine** out']
    assert 'ts2d_engine_create_residual' in _lib.SYMBOLS and 'ts2d_engine_create_residual' in _lib.OPTIONAL
    lib = _lib.load()
    assert hasattr(lib, 'ts2d_engine_create_residual')
    assert lib.ts2d_abi_version() == _lib.ABI_VERSION == 9                                # new symbols only
    c = ctypes
    assert lib.ts2d_engine_create_residual.restype is c.c_int
    assert lib.ts2d_engine_create_residual.argtypes == [c.POINTER(_lib.ArchDesc), c.POINTER(_lib.ResidualDesc), c.c_void_p, c.c_size_t, c.c_int,
                                                        c.POINTER(c.c_void_p)]
    # refused before any device work, by name
    h = c.c_void_p()
    assert lib.ts2d_engine_create_residual(c.byref(_lib.ArchDesc()), None, None, 0, 0, c.byref(h)) == -1
    assert 'ts2d_engine_create_residual' in _lib.last_error() and not h.value
    r = _lib.ResidualDesc()
    r.reserved[3] = 1
    assert lib.ts2d_engine_create_residual(c.byref(_lib.ArchDesc()), c.byref(r), None, 0, 0, c.byref(h)) == -1
    assert 'reserved' in _lib.last_error()


def test_the_model_folder_loader_ignores_the_duplicate_keys_of_a_real_checkpoint(tmp_path):
    arch = R.RES_CASES['res_pool'][0]
    blobs = []
    for dup in (False, True):
        root = tmp_path / f'dup{int(dup)}'
        root.mkdir()
        want = R.write_model_folder(str(root), arch, 41, (64, 64), dup)
        p = HostLogicPredictor(network=None)
        p.initialize_from_trained_model_folder(str(root), (0,), 'checkpoint_final.pth')
        assert p.arch == arch and p.arch.encoder == 'residual'
        assert len(p.list_of_parameters) == 1 and np.array_equal(p.list_of_parameters[0], want)
        blobs.append(p.list_of_parameters[0])
    assert np.array_equal(blobs[0], blobs[1]) and blobs[0].size == arch.n_params()


@pytest.mark.parametrize('extra, word', [({'bottleneck_channels': [8, 16, 16]}, 'bottleneck_channels'),
                                         ({'block': 'dynamic_network_architectures.building_blocks.residual.BottleneckD'}, 'BottleneckD'),
                                         ({'stem_channels': 16}, 'stem_channels'),
                                         ({'squeeze_excitation': True}, 'squeeze_excitation'),
                                         ({'conv_bias': False}, 'conv_bias')])
def test_unsupported_variants_are_refused_by_name(extra, word):
    arch = R.RES_CASES['res_pool'][0]
    with pytest.raises(NotImplementedError, match=word):
        UNetArch.from_plans(R.plans_for(arch, extra=extra), '2d', 2, 5).validate()
    # the supported spellings of the same keys pass
    ok = {'block': 'dynamic_network_architectures.building_blocks.residual.BasicBlockD', 'bottleneck_channels': None, 'stem_channels': 32,
          'squeeze_excitation': False}
    assert UNetArch.from_plans(R.plans_for(arch, extra=ok), '2d', 2, 5) == arch
