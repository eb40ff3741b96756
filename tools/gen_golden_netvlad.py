#!/usr/bin/env python3
"""Golden vectors for the NetVLAD text encoder (tests/golden/netvlad_text.npz), from the REAL reference.

Runs only in the build container: it reuses gen_golden.import_reference() (the stub recipe, by importing gen_golden), writes a small
seeded word2vec BigFile to a temporary directory, builds the reference's own W2VecNSW (txt2vec.py:145-149) over it with the stop words
given here as data (textlib.ENGLISH_STOP_WORDS is replaced for the run) and the reference's own NetVLADTxtEncoder
(model/model.py:529-549) on CPU for K = 8 and K = 32, and writes arrays and JSON strings only.

    python tools/gen_golden_netvlad.py
"""
import json
import os
import sys
import tempfile
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (imports the reference with its stubs; mm.device = cpu)

import numpy as np  # noqa: E402
import torch  # noqa: E402

D = 40
STOPWORDS = ['a', 'an', 'the', 'is', 'are', 'on', 'in', 'of', 'and', 'to', 'with', 'at', 'by']
KNOWN = ['man', 'woman', 'playing', 'guitar', 'stage', 'dog', 'cat', 'running', 'park', 'two', 'girls', 'dancing', 'singing',
         'cooking', 'food', 'kitchen', 'car', 'street', 'video', '3d', 'tv', 'news', 'zero'] + ['w%d' % i for i in range(130)]


def captions(g):
    caps = ['', '?!', 'the a an of', 'zebra unicorn quokka', 'A DOG running in the park!!!', 'dog dog cat dog cat',
            'a man is playing the guitar on the stage', 'two girls dancing & singing', "someone's 3D-TV news", 'zero',
            'zero dog', 'the zebra', 'cooking food in the kitchen\r\nvideo', 'car   street ', 'a cat', 'a cat']
    while len(caps) < 39:
        n = int(g.integers(1, 14))
        caps.append(' '.join(str(w) for w in g.choice(KNOWN[:22] + STOPWORDS + ['unknownword', 'Xyz'], n)))
    caps.append(' '.join(KNOWN[22:] + KNOWN[22:60]))                      # more than 100 distinct known words, some repeated
    return caps


def main():
    mm = G.mm
    import textlib as ref_textlib
    import txt2vec as ref_t2v
    g = G.rng(4242)
    caps = captions(g)
    words = KNOWN + STOPWORDS[:3]                                         # stop words in the table are still dropped
    table = G.f32(g.normal(0, 1, (len(words), D)))
    table[words.index('zero')] = 0.0                                      # a zero-norm row
    ref_textlib.ENGLISH_STOP_WORDS = set(STOPWORDS)
    arrays = {'captions': np.array(json.dumps(caps)), 'words': np.array(json.dumps(words)), 'stopwords': np.array(json.dumps(STOPWORDS)),
              'table': table}
    with tempfile.TemporaryDirectory() as d:
        table.tofile(os.path.join(d, 'feature.bin'))
        open(os.path.join(d, 'id.txt'), 'w').write(' '.join(words))
        open(os.path.join(d, 'shape.txt'), 'w').write('%d %d' % table.shape)
        t2v = ref_t2v.W2VecNSW(d)
        # raw_encoding's row set: the names BigFile.read returns (row order) and the number of rows (zero rows when none is known)
        raw = []
        for c in caps:
            names, _ = t2v.w2v.read(t2v._preprocess(c))
            x = t2v.raw_encoding(c)
            assert np.array_equal(x, table[[words.index(n) for n in names]]) if names else not x.any()
            raw.append([list(names), len(x)])
        arrays['raw'] = np.array(json.dumps(raw))
        for K in (8, 32):
            enc = mm.NetVLADTxtEncoder(types.SimpleNamespace(t2v_w2v=t2v, NetVLAD_opt={'num_clusters': K, 'alpha': 100})).eval()
            sd = {n: torch.from_numpy(G.f32(g.normal(0, 1.0 / np.sqrt(D), p.shape))) for n, p in enc.state_dict().items()}
            enc.load_state_dict(sd, strict=True)
            for n, v in sd.items():
                arrays['k%d/sd/%s' % (K, n)] = v.numpy()
            with torch.no_grad():
                arrays['k%d/out' % K] = enc({'caption': caps})['text_features'].numpy().astype(np.float32)
    G.save('netvlad_text', **arrays)


if __name__ == '__main__':
    main()
