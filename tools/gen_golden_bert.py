#!/usr/bin/env python3
"""Golden vectors for the BERT text encoder (tests/golden/bert_text.npz, tests/golden/bert_vocab.txt), from the REAL reference.

Runs only in the build container: it reuses gen_golden.import_reference() (the stub recipe, by importing gen_golden), writes a small
seeded BERT checkpoint (BertConfig: hidden 128, 2 heads, 2 layers, intermediate 512, 512 positions; a fixture vocab.txt of a few
hundred entries with the special tokens at their bert-base-uncased ids) into a temporary directory and runs the reference's own
BertTxtEncoder.forward on the captions with from_pretrained pointed there (BertTokenizer + BertModel, fp32, pooler_output).
It writes arrays and JSON strings only:
  captions (json), ids [N, Lmax] int32 and mask [N, Lmax] int8 (the reference tokenizer's padded batch), cfg (json),
  q/<name> int8 + e/<name> int8: every BertModel parameter as q * 2**e, |q| <= QMAX, pooler_output [N, 128] fp32.
The parameters are drawn at BertConfig's initializer range (LayerNorm affines and biases moved off 1 / 0) and rounded to that grid
BEFORE the reference runs, so the stored values are exactly the ones it saw, and the file stays small.

    python tools/gen_golden_bert.py
"""
import json
import os
import sys
import tempfile
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (imports the reference with its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

WIDTH, HEADS, LAYERS, INTER, MAXPOS = 128, 2, 2, 512, 512
QMAX = 31                                   # |q| of the stored grid: 6 bits of each drawn parameter

WORDS = ('the a an and of in on at to is are was with for from by his her their its it this that man woman men women person people '
         'boy girl girls child kids baby dog dogs cat cats bird horse car cars bike street road park kitchen stage guitar piano music '
         'song video game news anchor weather food cooking pasta water ball football basketball players team field play plays playing '
         'played dance dances dancing sing sings singing run runs running walk walking talk talking talks cut slicing tomato make '
         'makeup how about red blue green black white big small old young fast slow motion two three one hello world token cafe naive '
         'city zurich rock roll band live tv cartoon characters story tells quick brown fox jumps over lazy someone someones isn t '
         'they re sleeping barking we ll see what you ve done wow ok time lapse clouds lion hunting savanna explains tutorial printing')
SUFFIXES = ('s', 'ing', 'ed', 'er', 'ly', 'es', 'ist', 'ion')
CJK = '中文猫狗一只和'


def vocab_tokens():
    """[PAD] = 0, [unused0..98] = 1..99, [UNK] = 100, [CLS] = 101, [SEP] = 102, [MASK] = 103 (bert-base-uncased's ids), then single
    characters, '##' continuations and whole words."""
    toks = ['[PAD]'] + ['[unused%d]' % i for i in range(99)] + ['[UNK]', '[CLS]', '[SEP]', '[MASK]']
    chars = [chr(c) for c in range(33, 127) if not chr(c).isupper()] + list(CJK)
    toks += chars + ['##' + c for c in 'abcdefghijklmnopqrstuvwxyz0123456789'] + ['##' + s for s in SUFFIXES]
    for w in WORDS.split():
        if w not in toks:
            toks.append(w)
    return toks


CAPTIONS = [
    '', 'a man is playing the guitar on the stage', 'A DOG running in the park!!!', 'two girls dancing & singing',
    'a café in the naïve city of Zürich', 'ÀÉÎÕÜ accents Ñ everywhere', '一只猫和狗 play together', 'news中文anchor talks',
    'what?!?! ... wow --- ok ;;; :)', '(((nested))) [brackets] {braces} <tags>', 'hello [SEP] world', '[UNK] token [CLS]x[MASK]',
    'lower case [sep] is not special', 'the [PAD]dog', 'someone\'s dog isn\'t barking, they\'re sleeping',
    'a xylophonist plays', 'an emoji \U0001F642 cat', 'greek ω letters', 'tab\tnew\nline\r\nnbsp space',
    'control\x00chars\x07and�replacement', 'the ' + 'a' * 101 + ' dog', 'the ' + 'b' * 100 + ' cat',
    'the 3 cats and 1999 dogs', 'rock-n-roll band performs live on tv', 'cooking pasta in a kitchen', 'a baby laughing',
    'slow motion water', 'people walking on a busy street', 'a red car drives fast', 'basketball players 23 vs 45',
    'kids play football in the field', 'time-lapse of clouds', 'a lion hunting in the savanna', 'someone is slicing a tomato',
]


def long_caption():
    """Above 510 word pieces: cut to [CLS] + 510 + [SEP]."""
    return ' '.join(['the dog runs and jumps over the fence while a cat watches'] * 60)


def make_opt(local_dir):
    return types.SimpleNamespace(text_encoding={'bert_encoding': {'name': local_dir}}, bert_do_lower_case=True, bert_frozen=True)


def main():
    mm = G.mm
    import transformers
    caps = CAPTIONS + [long_caption()]
    toks = vocab_tokens()
    g = G.rng(8088)
    torch.manual_seed(8088)
    cfg = transformers.BertConfig(vocab_size=len(toks), hidden_size=WIDTH, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                                  intermediate_size=INTER, max_position_embeddings=MAXPOS, hidden_act='gelu', layer_norm_eps=1e-12)
    model = transformers.BertModel(cfg).eval()
    grid = {}
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith('bias'):                         # LayerNorm affines and biases away from their 1 / 0 init
                p.copy_(torch.from_numpy(G.f32(g.normal(0, 0.05, p.shape))))
            elif 'LayerNorm' in n:
                p.copy_(torch.from_numpy(G.f32(1 + g.normal(0, 0.1, p.shape))))
            e = int(np.ceil(np.log2(float(p.abs().max()) / QMAX)))   # onto the q * 2**e grid (int8 q, per-tensor exponent)
            q = torch.clamp(torch.round(p / 2.0 ** e), -QMAX, QMAX)
            p.copy_(q * 2.0 ** e)
            grid[n] = (q.numpy().astype(np.int8), np.int8(e))
    with tempfile.TemporaryDirectory() as d:
        model.save_pretrained(d)
        with open(os.path.join(d, 'vocab.txt'), 'w', encoding='utf-8') as f:
            f.write('\n'.join(toks) + '\n')
        with open(os.path.join(d, 'tokenizer_config.json'), 'w') as f:
            json.dump({'do_lower_case': True, 'model_max_length': MAXPOS}, f)
        enc = mm.BertTxtEncoder(make_opt(d)).eval()
        with torch.no_grad():
            out = enc({'caption': caps})['text_features'].numpy().astype(np.float32)
            batch = enc.tokenizer(caps, padding=True, truncation=True)
    ids, mask = np.array(batch['input_ids'], np.int32), np.array(batch['attention_mask'], np.int8)
    assert ids.shape[1] == MAXPOS and mask[-1].sum() == MAXPOS
    arrays = {'captions': np.array(json.dumps(caps)), 'ids': ids, 'mask': mask, 'pooler_output': out,
              'cfg': np.array(json.dumps({'hidden_size': WIDTH, 'num_attention_heads': HEADS, 'num_hidden_layers': LAYERS,
                                          'intermediate_size': INTER, 'max_position_embeddings': MAXPOS, 'vocab_size': len(toks),
                                          'type_vocab_size': 2, 'layer_norm_eps': 1e-12, 'hidden_act': 'gelu',
                                          'position_embedding_type': 'absolute'}))}
    for n, (q, e) in grid.items():
        arrays['q/' + n] = q
        arrays['e/' + n] = e
    G.save('bert_text', **arrays)
    dst = os.path.join(G.OUT, 'bert_vocab.txt')
    with open(dst, 'w', encoding='utf-8') as f:
        f.write('\n'.join(toks) + '\n')
    print('wrote %s (%d tokens)' % (dst, len(toks)))


if __name__ == '__main__':
    main()
