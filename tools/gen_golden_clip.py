#!/usr/bin/env python3
"""Golden vectors for the CLIP text encoder (tests/golden/clip_text.npz), from the REAL reference.

Runs only in the build container: it reuses gen_golden.import_reference() (the stub recipe, ftfy stubbed to the identity, by
importing gen_golden), builds the reference's own clip.model.CLIP on CPU at a small text config (width 128, 2 heads, 2 layers,
embed 64; context 77, the full 49,408-token vocabulary) with seeded parameters, tokenises the captions with the reference's
clip.tokenize and runs encode_text in fp32.  It writes arrays and JSON strings only:
  captions (json), ids [N, 77] int32 (clip.tokenize), cfg (json), tok_rows [U] int32 (the token-embedding rows the captions use),
  q/<name> int8 + e/<name> int8: every text parameter as q * 2**e, |q| <= QMAX (token_embedding.weight: its tok_rows only),
  encode_text [N, 64] fp32.  The parameters are drawn at CLIP's init scales and rounded to that grid BEFORE the reference runs,
  so the stored values are exactly the ones encode_text saw, and the file stays small.
Next to it, tests/golden/clip_bpe_subset.txt.gz: the CLIP merges file with every line that no BPE of the fixture captions, the test
captions and tools/bench_clip.py's words applies replaced by a placeholder merge that can never fire (U+4E00 twice: not a byte
symbol).  Every line keeps its position, so ranks and token ids are the full file's; the reference's own tokenizer, pointed at the
subset, must give the same ids on all those captions (checked here).

    python tools/gen_golden_clip.py
"""
import gzip
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (imports the reference with its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

WIDTH, HEADS, LAYERS, EMBED = 128, 2, 2, 64
QMAX = 31                                   # |q| of the stored grid: 6 bits of each drawn parameter

CAPTIONS = [
    '', 'a man is playing the guitar on the stage', 'A DOG running in the park!!!', 'two girls dancing &amp; singing',
    'tom &amp;amp; jerry &lt;b&gt;cartoon&lt;/b&gt;', "someone's dog isn't barking, they're sleeping", "we'll see what you've done",
    'the 3 cats and 1999 dogs', '12345 67890', 'what?!?! ... wow --- ok ;;; :)', 'a café in the naïve city of zürich',
    'a man is playing the guitar on the stage', 'a cat', 'a cat', '   spaces\tand\nnewlines\r\n everywhere   ',
    'snake_case and CamelCase words', 'email me at someone@example.com', 'C++ and C# programming tutorial',
    'the quick brown fox jumps over the lazy dog', 'Hello <|endoftext|> world', 'rock-n-roll band performs live on tv',
    'cooking pasta in a kitchen', 'a baby laughing', 'news anchor reports the weather', 'minecraft gameplay video',
    'slow motion water drop', 'people walking on a busy street', 'a red car drives fast', 'basketball players 23 vs 45',
    'a woman explains how to do makeup', 'kids play football in the yard', 'a bird sings', 'time-lapse of clouds',
    'an old man tells a story', 'cartoon characters talk', 'someone is slicing a tomato', 'music video with dancers',
    'a tutorial about 3d printing', 'a lion hunting in the savanna',
]


# the words of tests/test_gpu_clip.py and tools/bench_clip.py: the subset merges file tokenises them as the full one does
OTHER_TEXT = ("dog cat man playing guitar on the stage a red car is running 3d it's !! word woman plays dances in park kitchen news "
              "person are piano street blue two people dancing singing cooking food video of talking about game minecraft football "
              "basketball someone showing how to make cake water slow motion child baby laughing")
PLACEHOLDER = '\u4e00 \u4e00'


def long_caption():
    return ' '.join(['the dog runs and jumps over the fence while a cat watches from the window'] * 8)


def main():
    mm = G.mm
    from model.clip import model as cm
    tokenize = mm.clip.tokenize
    caps = CAPTIONS + [long_caption()]
    g = G.rng(7077)
    torch.manual_seed(7077)
    clip = cm.CLIP(EMBED, 32, 1, 64, 32, 77, 49408, WIDTH, HEADS, LAYERS).eval()
    with torch.no_grad():                                  # LayerNorm affines and biases away from their 1 / 0 init
        for n, p in clip.named_parameters():
            if n.startswith('visual.'):
                continue
            if n.endswith('bias'):
                p.copy_(torch.from_numpy(G.f32(g.normal(0, 0.05, p.shape))))
            elif '.ln_' in '.' + n and n.endswith('weight'):
                p.copy_(torch.from_numpy(G.f32(1 + g.normal(0, 0.1, p.shape))))
    with torch.no_grad():                                  # onto the q * 2**e grid (int8 q, per-tensor exponent)
        grid = {}
        for n, p in clip.named_parameters():
            if n.startswith('visual.') or n == 'logit_scale':
                continue
            e = int(np.ceil(np.log2(float(p.abs().max()) / QMAX)))
            q = torch.clamp(torch.round(p / 2.0 ** e), -QMAX, QMAX)
            p.copy_(q * 2.0 ** e)
            grid[n] = (q.numpy().astype(np.int8), np.int8(e))
    ids = tokenize(caps)
    with torch.no_grad():
        out = clip.encode_text(ids).numpy().astype(np.float32)
    rows = np.unique(ids.numpy())
    arrays = {'captions': np.array(json.dumps(caps)), 'ids': ids.numpy().astype(np.int32),
              'cfg': np.array(json.dumps({'width': WIDTH, 'heads': HEADS, 'layers': LAYERS, 'embed_dim': EMBED, 'context_length': 77,
                                          'vocab_size': 49408})),
              'tok_rows': rows.astype(np.int32), 'encode_text': out}
    for n, (q, e) in grid.items():
        arrays['q/' + n] = q[rows] if n == 'token_embedding.weight' else q
        arrays['e/' + n] = e
    G.save('clip_text', **arrays)
    write_bpe_subset(caps + [OTHER_TEXT])


def write_bpe_subset(texts):
    from model.clip import simple_tokenizer as st
    full = os.path.join(G.REF, 'model', 'clip', 'bpe_simple_vocab_16e6.txt.gz')
    tok = st.SimpleTokenizer(full)
    lines = gzip.open(full).read().decode('utf-8').split('\n')
    n_merges = 49152 - 256 - 2
    keep, emitted = set(), set()
    for text in texts:                                     # the reference's BPE loop, recording the merges it applies
        for piece in st.re.findall(tok.pat, st.whitespace_clean(st.basic_clean(text)).lower()):
            word = tuple(''.join(tok.byte_encoder[b] for b in piece.encode('utf-8')))
            word = word[:-1] + (word[-1] + '</w>',)
            while len(word) > 1:
                pairs = set(zip(word, word[1:]))
                best = min(pairs, key=lambda p: tok.bpe_ranks.get(p, float('inf')))
                if best not in tok.bpe_ranks:
                    break
                keep.add(tok.bpe_ranks[best])
                out, i = [], 0
                while i < len(word):
                    if i + 1 < len(word) and word[i] == best[0] and word[i + 1] == best[1]:
                        out.append(word[i] + word[i + 1])
                        i += 2
                    else:
                        out.append(word[i])
                        i += 1
                word = tuple(out)
            emitted.update(word)
    for r in range(n_merges):                              # every line that spells an emitted token: the vocabulary's last one wins
        if ''.join(lines[1 + r].split()) in emitted:
            keep.add(r)
    sub = [lines[0]] + [lines[1 + r] if r in keep else PLACEHOLDER for r in range(n_merges)]   # (the lines past them are unused)
    dst = os.path.join(G.OUT, 'clip_bpe_subset.txt.gz')
    with gzip.GzipFile(dst, 'wb', mtime=0) as f:
        f.write('\n'.join(sub).encode('utf-8'))
    check = st.SimpleTokenizer(dst)
    for text in texts:
        assert check.encode(text) == tok.encode(text), text
    print('wrote %s (%d of %d merges, %.1f KB)' % (dst, len(keep), n_merges, os.path.getsize(dst) / 1024))


if __name__ == '__main__':
    main()
