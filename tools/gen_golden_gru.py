#!/usr/bin/env python3
"""Golden vectors for the GRU caption encoder (tests/golden/gru_encoder.npz), from the REAL reference.

Runs only in the build container: it reuses gen_golden.import_reference() (the stub recipe, by importing gen_golden), builds the
reference's own GruTxtEncoder / BiGruTxtEncoder (model/model.py:323-396) on CPU over a small seeded 'gru' vocabulary
(textlib.Vocabulary, pickled to a temporary file for txt2vec.IndexVec) and writes arrays and JSON strings only.

    python tools/gen_golden_gru.py
"""
import json
import os
import pickle
import sys
import tempfile
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (imports the reference with its stubs; mm.device = cpu)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, WE_DIM = 64, 50
WORDS = ['a', 'man', 'woman', 'is', 'playing', 'the', 'guitar', 'on', 'stage', 'dog', 'cat', 'running', 'in', 'park', 'two',
         'girls', 'dancing', 'and', 'singing', 'cooking', 'food', 'kitchen', 'car', 'street', 'video', 'of', '3d', 'tv', 'news']


def captions(g):
    caps = ['', 'a man is playing the guitar on the stage', 'A DOG running in the park!!!', 'two girls dancing & singing',
            'zebra unicorn quokka', 'a cat', 'a cat', 'cooking food in the kitchen\r\nvideo', 'the the the', "someone's 3D-TV news",
            'a man is playing the guitar on the stage', '   car   street  ', '?!', 'video of a dog and a cat']
    while len(caps) < 39:
        n = int(g.integers(1, 16))
        caps.append(' '.join(str(w) for w in g.choice(WORDS + ['unknownword', 'Xyz'], n)))
    caps.append(' '.join(str(w) for w in g.choice(WORDS, 110)))          # more than 100 tokens
    return caps


def main():
    mm = G.mm
    import textlib as ref_textlib
    import txt2vec as ref_t2v
    g = G.rng(2323)
    caps = captions(g)
    voc = ref_textlib.Vocabulary('gru')
    for w in ['<pad>', '<start>', '<end>', '<unk>'] + WORDS:
        voc.add(w)
    arrays = {'vocab': np.array(json.dumps([voc.idx2word[i] for i in range(len(voc))])), 'captions': np.array(json.dumps(caps)),
              'cfg': np.array(json.dumps({'H': H, 'we_dim': WE_DIM}))}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'gru_5.pkl')
        pickle.dump(voc, open(path, 'wb'))
        t2v = ref_t2v.IndexVec(path)
        arrays['ids'] = np.array(json.dumps([[int(i) for i in t2v.encoding(c)] for c in caps]))
        k = 1.0 / H ** 0.5
        for bi, cls in ((False, mm.GruTxtEncoder), (True, mm.BiGruTxtEncoder)):
            net = 'bigru' if bi else 'gru'
            enc = None
            for pooling in ('mean', 'last', 'mean_last') if not bi else ('mean', 'last'):
                opt = types.SimpleNamespace(rnn_size=H, rnn_layer=1, we_dim=WE_DIM, pooling=pooling, t2v_idx=t2v)
                e = cls(opt).eval()
                if enc is None:         # seeded weights at torch's init scale, shared by every pooling of this net
                    sd = {n: torch.from_numpy(G.f32(g.normal(0, 1, p.shape) if n == 'we.weight' else g.uniform(-k, k, p.shape)))
                          for n, p in e.state_dict().items()}
                    enc = sd
                    for n, v in sd.items():
                        arrays['%s/sd/%s' % (net, n)] = v.numpy()
                e.load_state_dict(enc, strict=True)
                with torch.no_grad():
                    arrays['%s_%s' % (net, pooling)] = e({'caption': caps})['text_features'].numpy().astype(np.float32)
    G.save('gru_encoder', **arrays)


if __name__ == '__main__':
    main()
