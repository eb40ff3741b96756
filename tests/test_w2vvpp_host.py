"""W2VV++ concat towers without a GPU: registry, state-dict keys, segment order, refusals, header / library / binding agreement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from laff_amd.config import make_config
from laff_amd.model import get_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('W2VVPP', 'w2vpp_mutivis_attention', 'LAFF')


def concat_cfg(c, **over):
    kw = dict(batch_norm=c['batch_norm'], txt_attention='concat', vis_attention='concat')
    kw.update(over)
    return make_config(c['vid_dims'], c['txt_dims'], c['D'], 1, 'W2VVPP', **kw)


def tower_keys(model):
    return sorted(k for k in model.state_dict() if not k.startswith('txt_net.encoder.'))


def test_state_dict_keys_equal_the_reference_for_all_three_registry_keys(golden):
    g = golden('w2vvpp')
    assert tuple(g.json('registry_keys')) == KEYS
    for c in g.json('cases'):
        ref = sorted(g.sub(c['key'] + '/sd/').keys())
        assert ref == c['sd_keys'] and len(ref) == (14 if c['batch_norm'] else 4)
        for name in KEYS:
            model = get_model(name, 'cpu', concat_cfg(c))
            assert tower_keys(model) == ref, name
            assert type(model.vis_net).__name__ == 'VisTransformNet' and type(model.txt_net).__name__ == 'MultiScaleTxtNet'
            sd = {k: torch.from_numpy(np.array(v)) for k, v in g.sub(c['key'] + '/sd/').items()}
            holder = torch.nn.Module()
            holder.vis_net, holder.txt_net = model.vis_net, torch.nn.Module()
            holder.txt_net.transformer = model.txt_net.transformer
            holder.load_state_dict(sd, strict=True)
            assert model.txt_net.encoder.encoder_name_list == c['encoder_name_list']
            assert [n for n, _ in model.txt_net.encoder.encoder.named_children()] == c['encoder_name_list']
            assert model.opt.txt_fc_layers[0] == sum(c['txt_dims'].values()) == model.txt_net.transformer.fc1.in_features
            assert model.vis_net.fc1.in_features == sum(c['vid_dims'].values())


def test_encoder_order_is_the_reference_order_and_concat_is_honoured_per_side():
    cfg = make_config({'a': 8}, {'CLIP': 16, 'w2v': 6, 'bow': 5, 'rnn': 12, 'bert': 10, 'NetVLAD': 2}, 32, 1, 'W2VVPP', txt_attention='concat',
                      vis_attention='attention_noAveNoAverageMul')
    m = get_model('w2vpp_mutivis_attention', 'cpu', cfg)
    enc = m.txt_net.encoder
    assert enc.encoder_name_list == ['rnn_encoder', 'bert_encoder', 'bow_encoder', 'w2v_encoder', 'CLIP_encoder', 'NetVLAD_encoder']
    assert list(enc.space_dict.values()) == [12, 10, 5, 6, 16, 12] and m.opt.txt_fc_layers[0] == 61
    assert type(m.vis_net).__name__ == 'VisMutiTransformNetAddAttnetion' and type(m.txt_net).__name__ == 'MultiScaleTxtNet'
    cfg = make_config({'a': 8, 'b': 4}, {'bow': 5}, 32, 1, 'W2VVPP', vis_attention='concat', txt_attention='attention_noAveNoAverageMul')
    m = get_model('LAFF', 'cpu', cfg)
    assert type(m.vis_net).__name__ == 'VisTransformNet' and type(m.txt_net).__name__ == 'MultiScaleTxtEncoderAttention'
    assert m.vis_net.fc1.in_features == 12
    # the concatenated feature itself, as the reference's encoder returns it: encoder order, CSR densified
    cfg = make_config({'a': 8}, {'bow': 5, 'w2v': 3}, 32, 1, 'W2VVPP', txt_attention='concat', vis_attention='concat')
    enc = get_model('W2VVPP', 'cpu', cfg).txt_net.encoder          # (get_model points the module's device at the CPU)
    bow = torch.tensor([[0., 2, 0, 0, 1], [0, 0, 0, 0, 0]])
    w2v = torch.arange(6.).view(2, 3)
    cat = enc({'caption': ['x', 'y'], 'w2v_encoding': w2v, 'bow_encoding': bow.to_sparse_csr()})
    assert torch.equal(cat, torch.cat([bow, w2v], dim=1))
    with pytest.raises(ValueError, match="'w2v_encoder' has 2 columns"):
        enc.segments({'caption': ['x'], 'w2v_encoding': w2v[:, :2], 'bow_encoding': bow})


def test_refusals_of_the_registry():
    cfg = make_config({'a': 8}, {'bow': 5}, 32, 1, 'W2VVPP', txt_attention='concat', vis_attention='concat')
    m = get_model('W2VVPP', 'cpu', cfg)
    with pytest.raises(NotImplementedError, match='training step'):
        m(None)
    m.train()
    with pytest.raises(NotImplementedError, match='inference path only'):
        m.vis_net({'a': torch.zeros(2, 8)})
    with pytest.raises(NotImplementedError):
        get_model('End2EndClip', 'cpu', cfg)
    cfg.txt_fc_same_with_vis_fc = True
    for name in KEYS:
        with pytest.raises(NotImplementedError, match='txt_fc_same_with_vis_fc'):
            get_model(name, 'cpu', cfg)
    from laff_amd.config import config
    assert config.txt_fc_same_with_vis_fc is False


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    fake = 4096
    Seg, Prob = _lib.FcConcatSegment, _lib.FcConcatProblem

    def dense(Dk=32, col=0, ldx=None, X=fake):
        return Seg(X, Dk if ldx is None else ldx, None, None, None, None, 0, Dk, col)

    def sparse(Dk=32, col=0, ldwt=64, Wt=fake, indptr=fake, indices=fake):
        return Seg(None, 0, indptr, indices, None, Wt, ldwt, Dk, col)

    def run(segs, N=5, K=None, ldw=None, D=64, ldy=None, W=fake, Y=fake, act=1, bias=None, bn=(None, None), nseg=None, ctx=None):
        arr = (Seg * max(1, len(segs)))(*segs)
        K = sum(s.Dk for s in segs) if K is None else K
        p = Prob(arr if segs is not None else None, len(segs) if nseg is None else nseg, N, W, K, K if ldw is None else ldw, bias, bn[0], bn[1],
                 D, act, Y, D if ldy is None else ldy)
        rc = lib.laff_fc_concat_act_bn(ctx, C.byref(p))
        return rc, lib.laff_last_error()

    def refused(rc_msg, code, text):
        return rc_msg[0] == code and text in rc_msg[1]
    assert refused(run([dense()], nseg=0), -1, b'1 <= nseg <= 8')
    assert refused(run([dense(4, 4 * i) for i in range(9)]), -1, b'nseg=9')
    assert refused(run([dense()], N=-1), -1, b'negative N')
    assert refused(run([dense()], D=62), -2, b'D=62')
    assert refused(run([dense()], D=8196), -2, b'D=8196')
    assert refused(run([dense()], D=0), -2, b'D=0')
    assert refused(run([dense()], ldy=60), -2, b'ldy=60')
    assert refused(run([dense()], ldy=66), -2, b'ldy=66')
    assert refused(run([dense(Dk=0)], K=4), -2, b'width Dk=0')
    assert refused(run([dense(32, 0), dense(32, 16)], K=64), -2, b'segments 0 and 1 overlap')
    assert refused(run([dense(32, 0), sparse(8, 31)], K=64), -2, b'overlap')
    assert refused(run([dense(32, 40)], K=64), -2, b'outside W')
    assert refused(run([dense(32, -1)], K=64), -2, b'outside W')
    assert refused(run([dense(32, 0, ldx=31)]), -2, b'ldx=31')
    assert refused(run([dense()], ldw=31), -2, b'ldw=31')
    assert refused(run([sparse(ldwt=60)]), -2, b'ldwt=60')
    assert refused(run([sparse(ldwt=66)]), -2, b'ldwt=66')
    assert refused(run([sparse(Wt=4100)]), -3, b'Wt must be 16-byte aligned')
    assert refused(run([sparse(Wt=None)]), -1, b'null X and null indptr')
    assert refused(run([sparse(indices=None)]), -1, b'null X and null indptr')
    assert refused(run([dense()], W=None), -1, b'null W / Y')
    assert refused(run([dense()], Y=None), -1, b'null W / Y')
    assert refused(run([dense()], Y=4100), -3, b'Y must be 16-byte aligned')
    assert refused(run([dense()], act=7), -1, b'bad act 7')
    assert refused(run([dense()], bn=(fake, None)), -1, b'bn_scale/bn_shift must come together')
    assert refused(run([dense()]), -1, b'null ctx')                       # valid arguments: only then the ctx
    assert refused(run([sparse()], W=None), -1, b'null ctx')              # W is not needed when every segment is sparse
    assert refused(run([dense(30, 0), sparse(50, 30), dense(40, 80, ldx=44)]), -1, b'null ctx')
    assert lib.laff_fc_concat_act_bn(None, None) == -1 and b'null problem' in lib.laff_last_error()
    assert lib.laff_fc_concat_act_bn_grouped(None, None, 1) == -1 and b'bad problem list' in lib.laff_last_error()
    # the empty problem is not looked at any further; a list of empty problems is a no-op once there is a context
    assert refused(run([dense()], N=0, W=None, Y=None, D=3), -1, b'null ctx')


def test_concat_entry_points_in_header_library_and_binding_at_the_header_abi():
    from laff_amd import _lib, build
    text = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    # the ctypes structures have the fields of the header's structs, in order
    for cname, cls in (('laff_fc_concat_segment', _lib.FcConcatSegment), ('laff_fc_concat_problem', _lib.FcConcatProblem)):
        body = re.search(r'typedef struct \{([^}]*)\} %s;' % cname, text).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        names = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            first, *rest = decl.split(',')
            names.append(re.findall(r'(\w+)\s*$', first)[0])
            names += [r.strip().lstrip('*') for r in rest]
        assert names == [f[0] for f in cls._fields_], (cname, names)
    assert 'fc_concat.hip' in build.SOURCES


def test_fc_concat_kernel_has_no_spills_and_no_scratch(tmp_path):
    import subprocess
    from laff_amd import build
    src = os.path.join(build.CSRC, 'fc_concat.hip')
    r = subprocess.run([build.hipcc()] + build.FLAGS + ['-save-temps=obj', '-c', src, '-o', str(tmp_path / 'fc_concat.o')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    asm = [str(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith('gfx950.s')]
    assert len(asm) == 1
    text = open(asm[0]).read()
    names = re.findall(r'\.name:\s+(_ZN4laff\w*fc_concat_kernel\w*)', text)
    assert len(names) == 1, names
    meta = text[text.index('.name:           ' + names[0]):]
    assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0
    assert int(re.search(r'\.private_segment_fixed_size: (\d+)', meta).group(1)) == 0
    assert 'v_mfma_f32_32x32x2_f32' in text and 'global_load_lds_dwordx4' in text
