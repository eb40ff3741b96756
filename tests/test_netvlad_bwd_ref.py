"""The float64 checker of the NetVLAD backward (tests/netvlad_bwd_ref.py) against the reference module's own CPU autograd
(tests/golden/netvlad_train.npz, tools/gen_golden_netvlad_train.py) and against torch autograd on the clamped branches; the
differentiable switch of NetVLADTxtEncoder and the C entry points, all without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import netvlad_bwd_ref as B
from laff_amd import txt2vec as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('laff_netvlad_train_reserve_bytes', 'laff_netvlad_backward_workspace_bytes', 'laff_netvlad_encode_train',
               'laff_netvlad_backward')


def fixture_case(z, c):
    """Case c of netvlad_train.npz: (captions as row arrays, fc1, cent, d_out, the float64 results, the float32 results)."""
    p = 'c%d/' % c
    off = np.concatenate([[0], np.cumsum(z[p + 'lens'])])
    caps = [z[p + 'rows'][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return caps, z[p + 'fc1'], z[p + 'cent'], z[p + 'dout'], z.sub(p + 'f64/'), z.sub(p + 'f32/')


@pytest.mark.parametrize('c', range(4))
def test_numpy_backward_against_the_reference_autograd(golden, c):
    z = golden('netvlad_train')
    caps, fc1, cent, dout, f64, _ = fixture_case(z, c)
    assert any(not x.any() for x in caps) and f64['out'].dtype == np.float64
    out, d_fc1, d_cent = B.netvlad_backward(caps, fc1, cent, dout)
    for name, got in (('out', out), ('fc1.weight', d_fc1), ('centeroids', d_cent)):
        err = B.rel_err(got, f64[name])
        print('case %d %-10s %.2e' % (c, name, err))
        assert err <= 1e-12


@pytest.mark.parametrize('c', range(4))
def test_torch_restatement_is_the_reference_module(golden, c):
    """The restatement that the GPU tests take their float32 yardstick from gives the reference module's own bits in float32."""
    caps, fc1, cent, dout, f64, f32 = fixture_case(golden('netvlad_train'), c)
    got = B.torch_module_grads(caps, fc1, cent, dout, torch.float32)
    for name in ('out', 'fc1.weight', 'centeroids'):
        assert np.array_equal(got[name], f32[name].astype(np.float64)), name
    got = B.torch_module_grads(caps, fc1, cent, dout, torch.float64)
    assert all(B.rel_err(got[name], f64[name]) <= 1e-12 for name in got)


def test_clamped_branches_against_float64_autograd():
    """A zero centroid row and a caption of all-zero rows: u_k = 0 exactly, |u_k| is clamped and the derivative is dv / eps; and with
    every centroid zero |v| is clamped too.  Against torch autograd in float64, computed here."""
    g = np.random.default_rng(5)
    K, D = 4, 8
    fc1, dout = g.normal(0, 0.3, (K, D)), g.normal(0, 1, (3, K * D))
    for zero_rows in ([2], [0, 1, 2, 3]):
        cent = g.normal(0, 0.3, (K, D))
        cent[zero_rows] = 0.0
        caps = [g.normal(0, 1, (3, D)), np.zeros((2, D)), g.normal(0, 1, (1, D))]
        want = B.torch_module_grads(caps, fc1, cent, dout, torch.float64)
        out, d_fc1, d_cent = B.netvlad_backward(caps, fc1, cent, dout)
        assert not out[1].reshape(K, D)[zero_rows].any()
        assert np.abs(d_cent[zero_rows]).max() > 1e9                       # the d / eps branch was taken
        for name, got in (('out', out), ('fc1.weight', d_fc1), ('centeroids', d_cent)):
            assert B.rel_err(got, want[name]) <= 1e-12, name
    # an empty caption adds exactly nothing
    caps = [g.normal(0, 1, (3, D)), np.zeros((0, D))]
    a = B.netvlad_backward(caps, fc1, cent, dout[:2])
    b = B.netvlad_backward(caps[:1], fc1, cent, dout[:1])
    assert not a[0][1].any() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_differentiable_switch_constructs_on_the_cpu_with_the_reference_keys():
    w2v = T.W2Vec(['a', 'b'], np.zeros((2, 20), np.float32))
    enc = T.NetVLADTxtEncoder(w2v, num_clusters=5, device='cpu', differentiable=True)
    assert enc.differentiable and sorted(enc.state_dict()) == ['netvlad.centeroids', 'netvlad.fc1.weight']
    assert [tuple(p.shape) for p in enc.parameters()] == [(5, 20), (5, 20)] and all(p.requires_grad for p in enc.parameters())
    assert not T.NetVLADTxtEncoder(w2v, num_clusters=5, device='cpu').differentiable
    # a CPU encoder is refused by name before anything is launched
    with pytest.raises(RuntimeError, match='netvlad.fc1.weight is a CPU tensor'):
        enc.train()({'caption': ['a b']})
    with pytest.raises(TypeError, match='netvlad.fc1.weight is torch.float16'):
        enc.half()({'caption': ['a b']})


def test_new_entry_points_in_header_library_and_binding():
    """(Header, library and binding: test_cabi.py, ENTRY_POINTS.)"""
    from laff_amd import ops
    for s in NEW_SYMBOLS:
        assert hasattr(ops, s[len('laff_'):])


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    n = C.c_size_t()
    r256 = lambda b: (b + 255) // 256 * 256
    assert lib.laff_netvlad_train_reserve_bytes(128, 2000, 32, C.byref(n)) == 0
    assert n.value == r256(2000 * 32 * 4) + r256(2000 * 4) + 2 * r256(128 * 33 * 4)
    assert lib.laff_netvlad_train_reserve_bytes(0, 0, 8, C.byref(n)) == 0 and n.value == 0
    assert lib.laff_netvlad_train_reserve_bytes(1, 1, 65, C.byref(n)) == -5 and b'K=65' in lib.laff_last_error()
    assert lib.laff_netvlad_train_reserve_bytes(-1, 1, 8, C.byref(n)) == -1
    # 2000 rows: 32 chunks of 64; 128 captions: 8 chunks of 16
    assert lib.laff_netvlad_backward_workspace_bytes(128, 2000, 32, 500, C.byref(n)) == 0
    assert n.value == r256(128 * 32 * 500 * 4) + r256(128 * 32 * 4) + r256(2000 * 32 * 4) + (32 + 8) * r256(32 * 500 * 4)
    assert lib.laff_netvlad_backward_workspace_bytes(0, 0, 8, 20, C.byref(n)) == 0 and n.value == 0
    assert lib.laff_netvlad_backward_workspace_bytes(1, 1, 8, 6, C.byref(n)) == -5 and b'D=6' in lib.laff_last_error()
    fake = C.c_void_p(4096)                                              # never dereferenced: every call below fails its checks first
    big = 1 << 30

    def enc(K=32, D=500, ro=(0, 3, 5), ldo=None, reserve=fake, reserve_bytes=big, ws=None):
        roh = (C.c_int * len(ro))(*ro)
        return lib.laff_netvlad_encode_train(None, fake, 100, D, fake, fake, roh, fake, len(ro) - 1, ro[-1], fake, fake, K, fake,
                                             K * D if ldo is None else ldo, reserve, reserve_bytes, ws, 0)

    def bwd(K=32, D=500, ro=(0, 3, 5), ldg=None, reserve_bytes=big, ws=fake, ws_bytes=big, d_fc1=fake, d_cent=fake, d_out=fake):
        roh = (C.c_int * len(ro))(*ro)
        return lib.laff_netvlad_backward(None, fake, 100, D, fake, fake, roh, fake, len(ro) - 1, ro[-1], fake, fake, K, fake, K * D,
                                         d_out, K * D if ldg is None else ldg, fake, reserve_bytes, d_fc1, d_cent, ws, ws_bytes)
    for call, name in ((enc, b'laff_netvlad_encode_train'), (bwd, b'laff_netvlad_backward')):
        assert call(K=65) == -5 and b'K=65' in lib.laff_last_error()
        assert call(D=6) == -5 and b'D=6' in lib.laff_last_error()
        assert call(ro=(0, 3, 2)) == -1 and b'decreases at caption 1' in lib.laff_last_error()
        assert call(reserve_bytes=64) == -1 and b'reserve too small' in lib.laff_last_error()
        assert call() == -1 and name + b': null ctx' in lib.laff_last_error()      # valid arguments: only then the ctx
    assert enc(reserve=None) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(ldo=100) == -2 and b'ldo' in lib.laff_last_error()
    assert enc(ws=C.c_void_p(4100)) == -3 and b'aligned' in lib.laff_last_error()
    assert enc(ro=(0,)) == 0                                             # the empty problem: nothing to save
    assert bwd(ldg=32 * 500 + 2) == -2 and b'ldg' in lib.laff_last_error()
    assert bwd(ws_bytes=1 << 16) == -1 and b'workspace too small' in lib.laff_last_error()
    assert bwd(d_out=None) == -1 and b'null argument' in lib.laff_last_error()
    assert bwd(d_fc1=C.c_void_p(4100)) == -3 and b'd_fc1' in lib.laff_last_error()
    assert bwd(d_fc1=None, d_cent=None) == 0                             # nothing wanted: nothing to launch
    assert bwd(d_fc1=None) == -1 and b'null ctx' in lib.laff_last_error()
    assert bwd(ro=(0,), d_out=None, ws=None, ws_bytes=0) == -1 and b'null ctx' in lib.laff_last_error()   # N = 0: zeros are written


def test_netvlad_bwd_hip_kernels_have_no_scratch(tmp_path):
    """The saving pooling kernel and the three backward kernels of netvlad_bwd.hip: wave64, no VGPR spills and no scratch."""
    import subprocess
    from laff_amd import build
    src = os.path.join(build.CSRC, 'netvlad_bwd.hip')
    r = subprocess.run([build.hipcc()] + build.FLAGS + ['-save-temps=obj', '-c', src, '-o', str(tmp_path / 'netvlad_bwd.o')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    asm = [str(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith('gfx950.s')]
    assert len(asm) == 1
    text = open(asm[0]).read()
    names = re.findall(r'\.name:\s+(_ZN4laff\w*netvlad\w*)', text)
    assert len(names) == 4, names
    for name in names:
        meta = text[text.index('.name:           ' + name):]
        assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.private_segment_fixed_size: (\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.wavefront_size: (\d+)', meta).group(1)) == 64, name
