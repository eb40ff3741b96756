"""The NetVLAD text encoder's host side, without a GPU: captions -> table rows (the reference's W2VecNSW.raw_encoding row sets), the
float64 restatement against the reference's NetVLADTxtEncoder, the module's state-dict names, the make_config key, and the C entry
points' argument checks and ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from netvlad_ref import netvlad_features
from laff_amd import txt2vec as T


def fixture_w2v(z):
    return T.W2Vec(z.json('words'), z['table'], stopwords=z.json('stopwords'))


def test_raw_ids_are_the_reference_row_sets(golden):
    """Distinct known words in table-row order, stop words dropped (even those in the table), and the zero-row count of a caption
    whose words are all unknown."""
    z = golden('netvlad_text')
    w2v, words = fixture_w2v(z), z.json('words')
    caps, raw = z.json('captions'), z.json('raw')
    assert len(caps) == len(raw) >= 40
    for c, (names, nrows) in zip(caps, raw):
        ids, ntok = w2v.raw_ids(c)
        assert ids == [words.index(n) for n in names], c
        assert (len(ids) if ids else ntok) == nrows, c
    by = dict(zip(caps, raw))
    assert by[''] == [[], 0] and by['?!'] == [[], 0] and by['the a an of'] == [[], 0]
    assert by['zebra unicorn quokka'] == [[], 3] and by['the zebra'] == [[], 1]
    assert by['dog dog cat dog cat'] == [['dog', 'cat'], 2]
    assert len(raw[-1][0]) > 100


def test_ragged_layout(golden):
    z = golden('netvlad_text')
    w2v = fixture_w2v(z)
    caps = z.json('captions')
    ids, row_off, zero_rows = w2v.ragged(caps)
    assert ids.dtype == row_off.dtype == zero_rows.dtype == np.int32
    assert row_off.shape == (len(caps) + 1,) and row_off[0] == 0 and row_off[-1] == len(ids)
    for i, c in enumerate(caps):
        r, n = w2v.raw_ids(c)
        assert ids[row_off[i]:row_off[i + 1]].tolist() == r
        assert zero_rows[i] == (0 if r else n)
    e = w2v.ragged([])
    assert e[0].shape == (0,) and e[1].tolist() == [0] and e[2].shape == (0,)


def test_w2v_encoding_and_csr_are_unchanged(golden):
    """The mean-pooled w2v path keeps its values: the new helper only adds the token count."""
    z = golden('netvlad_text')
    w2v = fixture_w2v(z)
    table = z['table'].astype(np.float64)
    for c in z.json('captions'):
        ids, wts = w2v._ids(c)
        assert wts == [1.0 / max(1, len(ids))] * len(ids)
        want = table[ids].mean(0) if ids else np.zeros(table.shape[1])
        assert np.abs(w2v.encoding(c) - want).max() <= 1e-12


@pytest.mark.parametrize('K', [8, 32])
def test_float64_restatement_reproduces_the_reference(golden, K):
    z = golden('netvlad_text')
    w2v = fixture_w2v(z)
    sd = z.sub('k%d/sd/' % K)
    got = netvlad_features([w2v.raw_ids(c) for c in z.json('captions')], z['table'], sd['netvlad.fc1.weight'], sd['netvlad.centeroids'])
    want = z['k%d/out' % K]
    assert got.shape == want.shape == (40, K * 40)
    assert np.abs(got - want).max() <= 1e-6
    caps = z.json('captions')
    for c in ('', '?!', 'the a an of'):                                  # no rows: a zero row
        assert not want[caps.index(c)].any()
    c = sd['netvlad.centeroids'].astype(np.float64)                        # only unknown words: -c_k / |c_k| / sqrt(K)
    unk = -(c / np.linalg.norm(c, axis=1, keepdims=True)).reshape(-1) / np.sqrt(K)
    assert np.abs(want[caps.index('zebra unicorn quokka')] - unk).max() <= 1e-6
    assert np.abs(want[caps.index('the zebra')] - unk).max() <= 1e-6


def test_state_dict_names_match_the_reference(golden):
    z = golden('netvlad_text')
    enc = T.NetVLADTxtEncoder(fixture_w2v(z), num_clusters=32, alpha=100, device='cpu')
    sd = enc.state_dict()
    assert sorted(sd) == sorted(z.sub('k32/sd/')) == ['netvlad.centeroids', 'netvlad.fc1.weight']
    assert tuple(sd['netvlad.fc1.weight'].shape) == tuple(sd['netvlad.centeroids'].shape) == (32, 40)
    assert enc.netvlad.alpha == 100 and enc.netvlad.fc1.bias is None
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in z.sub('k32/sd/').items()}, strict=True)
    assert torch.equal(enc.netvlad.centeroids.detach(), torch.from_numpy(z['k32/sd/netvlad.centeroids']))


def test_encoder_refuses_unsupported_shapes():
    w2v = T.W2Vec(['a', 'b'], np.zeros((2, 40), np.float32))
    with pytest.raises(NotImplementedError, match='num_clusters=65'):
        T.NetVLADTxtEncoder(w2v, num_clusters=65, device='cpu')
    with pytest.raises(NotImplementedError, match='num_clusters=0'):
        T.NetVLADTxtEncoder(w2v, num_clusters=0, device='cpu')
    with pytest.raises(NotImplementedError, match='width 42'):
        T.NetVLADTxtEncoder(T.W2Vec(['a'], np.zeros((1, 42), np.float32)), device='cpu')
    with pytest.raises(NotImplementedError, match='width 1028'):
        T.NetVLADTxtEncoder(T.W2Vec(['a'], np.zeros((1, 1028), np.float32)), device='cpu')


def test_make_config_netvlad_key_is_additive():
    from laff_amd.config import make_config
    from laff_amd.model.model import MultiScaleTxtEncoderAttention
    base = make_config({'x': 8}, {'w2v': 20, 'CLIP': 512}, 64, 4)
    assert base.text_encoding['NetVLAD_encoding']['name'] == 'noNetVLAD' and 'NetVLAD_opt' not in vars(base)
    c = make_config({'x': 8}, {'w2v': 20, 'CLIP': 512, 'NetVLAD': 8}, 64, 4)
    assert c.text_encoding['NetVLAD_encoding']['name'] == 'NetVLAD' and c.NetVLAD_opt['num_clusters'] == 8
    t = MultiScaleTxtEncoderAttention(c)
    assert t.space_dict['NetVLAD_encoder'] == 160 and t.encoder_name_list[-1] == 'NetVLAD_encoder'


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.laff_netvlad_workspace_bytes(1000, 32, C.byref(n)) == 0 and n.value == 128000 + 4096
    assert lib.laff_netvlad_workspace_bytes(0, 8, C.byref(n)) == 0 and n.value == 0
    assert lib.laff_netvlad_workspace_bytes(10, 65, C.byref(n)) == -5 and b'K=65' in lib.laff_last_error()
    assert lib.laff_netvlad_workspace_bytes(-1, 8, C.byref(n)) == -1
    fake = C.c_void_p(4096)                                              # never dereferenced: every call below fails its checks first

    def enc(K=32, D=500, V=100, ro=(0, 3, 5), R=None, ldo=None, ids=fake, zr=fake, table=fake, out=fake, ws=fake, ws_bytes=1 << 30):
        roh = (C.c_int * len(ro))(*ro)
        return lib.laff_netvlad_encode(None, table, V, D, ids, fake, roh, zr, len(ro) - 1, ro[-1] if R is None else R, fake, fake, K,
                                       out, K * D if ldo is None else ldo, ws, ws_bytes)
    assert enc(K=0) == -5 and b'K=0' in lib.laff_last_error()
    assert enc(K=65) == -5 and b'K=65' in lib.laff_last_error()
    assert enc(D=502) == -5 and b'D=502' in lib.laff_last_error()
    assert enc(D=1028) == -5 and b'D=1028' in lib.laff_last_error()
    assert enc(D=0) == -5
    assert enc(V=0) == -2 and b'V=0' in lib.laff_last_error()
    assert enc(ro=(1, 3, 5)) == -1 and b'row_off[0]' in lib.laff_last_error()
    assert enc(ro=(0, 3, 2)) == -1 and b'decreases at caption 1' in lib.laff_last_error()
    assert enc(ro=(0, 3, 5), R=6) == -1 and b'row_off[N]=5 != R=6' in lib.laff_last_error()
    assert enc(ids=None) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(zr=None) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(table=None) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(ldo=32 * 500 - 4) == -2 and b'ldo' in lib.laff_last_error()
    assert enc(ldo=32 * 500 + 2) == -2 and b'ldo' in lib.laff_last_error()
    assert enc(ws_bytes=16) == -1 and b'workspace too small' in lib.laff_last_error()
    assert enc(out=C.c_void_p(4100)) == -3 and b'aligned' in lib.laff_last_error()
    assert enc() == -1 and b'null ctx' in lib.laff_last_error()         # valid arguments: only then the ctx
    assert enc(ro=(0,)) == 0                                            # the empty problem
    assert enc(ro=(0, 0, 0), ids=None, ws=None, ws_bytes=0) == -1 and b'null ctx' in lib.laff_last_error()   # no ids: none read


def test_netvlad_hip_kernels_have_no_scratch(tmp_path):
    """Every netvlad_* kernel of netvlad.hip: no VGPR spills and no scratch."""
    import subprocess
    from laff_amd import build
    src = os.path.join(build.CSRC, 'netvlad.hip')
    r = subprocess.run([build.hipcc()] + build.FLAGS + ['-save-temps=obj', '-c', src, '-o', str(tmp_path / 'netvlad.o')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    asm = [str(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith('gfx950.s')]
    assert len(asm) == 1
    text = open(asm[0]).read()
    names = re.findall(r'\.name:\s+(_ZN4laff\w*netvlad\w*)', text)
    assert len(names) == 5, names                                         # 4 assign widths (K <= 8, 16, 32, 64) + the VLAD kernel
    for name in names:
        meta = text[text.index('.name:           ' + name):]
        assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.private_segment_fixed_size: (\d+)', meta).group(1)) == 0, name
