"""Word n-gram language model read from an ARPA text file (plain or gzip), without kenlm -- the model behind
GPUPrefixBeamSearchLMDecoder and a host scorer for beam_search.prefix_beam_search (``lm=lambda s: 10 ** lm.score(s)``
stands in for the reference's ``lm_weigh``, decoder.py:240-243).

Scoring (ArpaLM.score) follows kenlm.Model.score's interface and, as far as can be determined without kenlm, its
arithmetic.  For a word w after the history h_1 (most recent) .. h_m (m <= order - 1):

    j = the largest length for which h_j .. h_1 w is a real n-gram (an OOV word is <unk>, so j >= 0)
    q(w | h) = prob(h_j .. h_1 w) + bo(h_{j+1} .. h_1) + ... + bo(h_m .. h_1)

all log10 values as float32, the backoffs added in order of increasing context length (an absent context adds 0), and the
sentence total a float32 running sum, word by word, then </s>.  score() is written by this definition with dicts of
tuples; it is the oracle of the device tables (to_device) and of the device beam search.

Device layout (ArpaLM.flat_tables / to_device).  Every n-gram gets a global entry index, unigrams their word id.  The entry
of h_2 h_1 w is found from the entry of h_1 w and the word h_2 through an open-addressing table keyed by the exact 64-bit
pair (parent entry << 32 | word id), so a walk w -> h_1 w -> h_2 h_1 w ... yields both the longest match of q(w | h) and
the backoffs of the next state's contexts (kenlm's state design).  For the walk to stop at the first missing entry, the
model is suffix-closed: an n-gram whose suffix (oldest word dropped) is absent gets that suffix as a context-only entry (no
probability of its own: NaN; backoff 0), counted in ``stats['context_only']``.  A spelling trie over the vocabulary words
that the labels can spell, keyed by the exact pair (trie node << 8 | canonical label), maps a partial word to its word id."""
from __future__ import annotations

import ctypes as C
import gzip
import math
import re
import time
from typing import Dict, List, Sequence, Tuple

import numpy as np

MAX_ORDER = 6
UNK, BOS, EOS = 0, 1, 2
_F32 = np.float32
_NGRAM_RE = re.compile(r'ngram\s+(\d+)\s*=\s*(\d+)')
_SECTION_RE = re.compile(r'\\(\d+)-grams:')


def _open(path):
    with open(path, 'rb') as f:
        head = f.read(8)
    gz = head[:2] == b'\x1f\x8b'
    if gz:
        with gzip.open(path, 'rb') as f:
            head = f.read(8)
    if head.startswith(b'mmap lm '):
        raise ValueError('%s, line 1: a kenlm binary model; convert to ARPA (kenlm has no loader here)' % path)
    return gzip.open(path, 'rt', encoding='utf-8') if gz else open(path, 'r', encoding='utf-8')


def table_capacity(n: int) -> int:
    """power-of-two capacity of an open-addressing table for n keys at load factor <= 0.5"""
    cap = 16
    while cap < 2 * n:
        cap <<= 1
    return cap


def build_spelling_trie(words, labels: Sequence[str], blank_index: int = 0):
    """the flat spelling trie of ``words`` (pairs (id, word), in insertion order) over ``labels``: (keys uint64 (node << 8 |
    canonical label), vals int32 (child node), word int32 [nodes] (the id a node spells, -1), the number of words dropped).  A
    word is dropped when one of its characters is not a label, is the blank's character or is whitespace; a duplicate
    label spells with its first index.  Shared by ArpaLM.spelling_trie and lexicon.Lexicon.spelling_trie."""
    labels = list(labels)
    first: Dict[str, int] = {}
    for i, ch in enumerate(labels):
        first.setdefault(ch, i)
    first.pop(labels[blank_index], None)
    children: Dict[Tuple[int, int], int] = {}
    word = [-1]
    dropped = 0
    for wid, w in words:
        if not all(ch in first and not ch.isspace() for ch in w):
            dropped += 1
            continue
        node = 0
        for ch in w:
            key = (node, first[ch])
            child = children.get(key)
            if child is None:
                child = children[key] = len(word)
                word.append(-1)
            node = child
        word[node] = wid
    keys = np.array([(nd << 8) | c for nd, c in children], dtype=np.uint64)
    vals = np.array(list(children.values()), dtype=np.int32)
    return keys, vals, np.array(word, dtype=np.int32), dropped


class ArpaLM:
    """An ARPA n-gram model (order <= 6).  Word ids: <unk> = 0, <s> = 1, </s> = 2, then the file's unigram order."""

    def __init__(self, path):
        self.path = str(path)
        self.words: List[str] = ['<unk>', '<s>', '</s>']
        self.vocab: Dict[str, int] = {w: i for i, w in enumerate(self.words)}
        self.warnings: List[str] = []
        # per order: word-id tuple (oldest word first) -> (log10 prob as a float32 value, NaN: context-only; log10 backoff)
        self.ngrams: List[Dict[Tuple[int, ...], Tuple[float, float]]] = []
        self._parse()
        self.order = len(self.ngrams)
        self._all: Dict[Tuple[int, ...], Tuple[float, float]] = {}
        for d in self.ngrams:
            self._all.update(d)
        self._flat = None
        self._tries: Dict[tuple, tuple] = {}
        self._device: Dict[tuple, 'DeviceLM'] = {}

    # ------------------------------------------------------------------------------------------------------------ parse
    def _parse(self):
        counts: Dict[int, int] = {}
        cur, seen, ended, lineno = 0, 0, False, 0
        unigram_seen = set()
        where = lambda: '%s, line %d' % (self.path, lineno)       # noqa: E731

        def close_section():
            if cur and seen != counts[cur]:
                raise ValueError('%s: %d-grams: the header announces %d, the section holds %d' % (where(), cur, counts[cur],
                                                                                                   seen))
        with _open(self.path) as f:
            state = 'pre'
            for raw in f:
                lineno += 1
                line = raw.strip()
                if state == 'pre':
                    if line == '\\data\\':
                        state = 'data'
                    continue
                if not line:
                    continue
                if state == 'data' and line.startswith('ngram'):
                    m = _NGRAM_RE.fullmatch(line)
                    if not m:
                        raise ValueError('%s: bad count line %r' % (where(), line))
                    n, c = int(m.group(1)), int(m.group(2))
                    if n > MAX_ORDER:
                        raise ValueError('%s: order %d > %d is not supported' % (where(), n, MAX_ORDER))
                    if n != len(counts) + 1:
                        raise ValueError('%s: ngram %d out of order' % (where(), n))
                    counts[n] = c
                    continue
                m = _SECTION_RE.fullmatch(line)
                if m:
                    close_section()
                    n = int(m.group(1))
                    if n != cur + 1 or n not in counts:
                        raise ValueError('%s: unexpected section \\%d-grams:' % (where(), n))
                    cur, seen, state = n, 0, 'grams'
                    self.ngrams.append({})
                    continue
                if line == '\\end\\':
                    close_section()
                    if cur != len(counts) or not counts:
                        raise ValueError('%s: \\end\\ before all %d sections' % (where(), len(counts)))
                    ended = True
                    break
                if state != 'grams':
                    raise ValueError('%s: unexpected line %r' % (where(), line))
                fields = line.split()
                top = cur == len(counts)
                if len(fields) == cur + 1:
                    bo = 0.0
                elif len(fields) == cur + 2 and not top:
                    bo = float(_F32(fields[-1]))
                else:
                    raise ValueError('%s: a %d-gram line needs %s fields, got %d' % (where(), cur, cur + 1 if top else
                                                                                   '%d or %d' % (cur + 1, cur + 2), len(fields)))
                try:
                    prob = float(_F32(fields[0]))
                except ValueError:
                    raise ValueError('%s: bad log10 probability %r' % (where(), fields[0])) from None
                seen += 1
                if seen > counts[cur]:
                    raise ValueError('%s: %d-grams: more than the %d announced' % (where(), cur, counts[cur]))
                toks = fields[1:cur + 1]
                if cur == 1:
                    w = toks[0]
                    if w in unigram_seen:
                        raise ValueError('%s: duplicate unigram %r' % (where(), w))
                    unigram_seen.add(w)
                    wid = self.vocab.get(w)
                    if wid is None:
                        wid = self.vocab[w] = len(self.words)
                        self.words.append(w)
                    self.ngrams[0][(wid,)] = (prob, bo)
                    continue
                try:
                    key = tuple(self.vocab[w] for w in toks)
                except KeyError as e:
                    raise ValueError('%s: word %s is not a unigram' % (where(), e)) from None
                if key in self.ngrams[cur - 1]:
                    raise ValueError('%s: duplicate %d-gram %r' % (where(), cur, ' '.join(toks)))
                self.ngrams[cur - 1][key] = (prob, bo)
        if state == 'pre':
            raise ValueError('%s: no \\data\\ header' % where())
        if not ended:
            raise ValueError('%s: truncated file (no \\end\\)' % where())
        for w in ('<s>', '</s>'):
            if (self.vocab[w],) not in self.ngrams[0]:
                raise ValueError('%s: the model has no %s unigram' % (where(), w))
        if (UNK,) not in self.ngrams[0]:
            self.ngrams[0][(UNK,)] = (float(_F32(-100.0)), 0.0)
            self.warnings.append('%s: no <unk>: log10 prob -100, backoff 0 (as kenlm)' % self.path)
        # suffix closure, highest order first so that inserted entries are closed in turn
        inserted = 0
        for n in range(len(self.ngrams), 2, -1):
            lower = self.ngrams[n - 2]
            for key in self.ngrams[n - 1]:
                if key[1:] not in lower:
                    lower[key[1:]] = (math.nan, 0.0)
                    inserted += 1
        self.stats = dict(order=len(self.ngrams), counts=[counts[n] for n in sorted(counts)], vocab=len(self.words),
                          context_only=inserted)

    # ------------------------------------------------------------------------------------------------------------ score
    def _real(self, key):
        e = self._all.get(key)
        return e is not None and e[0] == e[0]

    def q(self, w: int, hist: Sequence[int]) -> np.float32:
        """log10 q(w | hist) by the definition above; hist: word ids, most recent first, at most order - 1"""
        m = len(hist)
        j = m
        while not self._real(tuple(reversed(hist[:j])) + (w,)):
            j -= 1
        v = _F32(self._all[tuple(reversed(hist[:j])) + (w,)][0])
        for n in range(j + 1, m + 1):
            e = self._all.get(tuple(reversed(hist[:n])))
            v = _F32(v + _F32(e[1] if e is not None else 0.0))
        return v

    def score(self, sentence: str, bos: bool = True, eos: bool = True) -> float:
        """log10 probability of the words of ``sentence`` (str.split()), kenlm.Model.score's interface"""
        keep = self.order - 1
        hist = [BOS][:keep] if bos else []
        total = _F32(0.0)
        for word in sentence.split():
            w = self.vocab.get(word, UNK)
            total = _F32(total + self.q(w, hist))
            hist = ([w] + hist)[:keep]
        if eos:
            total = _F32(total + self.q(EOS, hist))
        return float(total)

    # ----------------------------------------------------------------------------------------------------- flat tables
    def flat_tables(self):
        """the n-gram entries in reverse-suffix form: dict(prob, bo, parent: [entries], keys: uint64 / vals: int32 of the
        entries of order >= 2 (key = parent entry << 32 | oldest word id, value = entry index)); unigram entry = word id"""
        if self._flat is not None:
            return self._flat
        vocab = len(self.words)
        n_entries = sum(len(d) for d in self.ngrams)
        if n_entries >= 1 << 30:
            raise ValueError('%s: %d n-gram entries, at most 2^30 are supported' % (self.path, n_entries))
        prob = np.empty(n_entries, dtype=np.float32)
        bo = np.empty(n_entries, dtype=np.float32)
        parent = np.full(n_entries, -1, dtype=np.int32)
        for (w,), (p, b) in self.ngrams[0].items():
            prob[w], bo[w] = p, b
        index: Dict[Tuple[int, ...], int] = {}
        nxt = vocab
        for n in range(2, self.order + 1):
            for key, (p, b) in self.ngrams[n - 1].items():
                index[key] = nxt
                prob[nxt], bo[nxt] = p, b
                parent[nxt] = key[1] if n == 2 else index[key[1:]]
                nxt += 1
        first = np.array([key[0] for n in range(2, self.order + 1) for key in self.ngrams[n - 1]], dtype=np.uint64)
        keys = (parent[vocab:].astype(np.uint64) << np.uint64(32)) | first
        vals = np.arange(vocab, n_entries, dtype=np.int32)
        self._flat = dict(prob=prob, bo=bo, parent=parent, keys=keys, vals=vals, vocab=vocab)
        return self._flat

    def spelling_trie(self, labels: Sequence[str], blank_index: int = 0):
        """(keys uint64 (node << 8 | canonical label), vals int32 (child node), word int32 [nodes] (word id, -1)): the
        vocabulary words every character of which is a label other than the blank's and not whitespace"""
        labels = list(labels)
        ck = (tuple(labels), blank_index)
        if ck in self._tries:
            return self._tries[ck]
        out = build_spelling_trie(enumerate(self.words), labels, blank_index)[:3]
        self._tries[ck] = out
        return out

    # ----------------------------------------------------------------------------------------------------------- device
    def to_device(self, labels: Sequence[str], blank_index: int = 0, device=None) -> 'DeviceLM':
        """the two hash tables (n-gram entries, spelling trie) built on the device by w2l_ngram_lm_build; cached per
        (labels, blank, device)"""
        import torch
        dev = torch.device(device if device is not None else 'cuda')
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        ck = (tuple(labels), blank_index, str(dev))
        if ck not in self._device:
            self._device[ck] = DeviceLM(self, list(labels), blank_index, dev)
        return self._device[ck]


class DeviceLM:
    """device tensors of one ArpaLM for one label set (w2l_ngram_lm_t); ``build_ms``: host-to-device copies and the two
    table insertions, wall time to completion"""

    def __init__(self, lm: ArpaLM, labels, blank_index, dev):
        import torch
        from ._lib import LmTables, check, lib, ptr, stream_ptr
        self.order = lm.order
        flat = lm.flat_tables()
        tkeys, tvals, tword = lm.spelling_trie(labels, blank_index)
        t0 = time.perf_counter()
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        self.prob, self.bo = to(flat['prob']), to(flat['bo'])
        self.trie_word = to(tword)
        dups = torch.zeros(1, dtype=torch.int32, device=dev)
        self.tables = []
        for keys, vals in ((flat['keys'], flat['vals']), (tkeys, tvals)):
            cap = table_capacity(len(keys))
            tk = torch.empty(cap, dtype=torch.int64, device=dev)
            tv = torch.empty(cap, dtype=torch.int32, device=dev)
            k_dev, v_dev = to(keys.view(np.int64)), to(vals)
            check(lib.w2l_ngram_lm_build(ptr(k_dev), ptr(v_dev), len(keys), ptr(tk), ptr(tv), cap, ptr(dups), stream_ptr()),
                  'w2l_ngram_lm_build')
            self.tables.append((tk, tv, cap))
        n_dups = int(dups.item())                              # (synchronises)
        self.build_ms = (time.perf_counter() - t0) * 1e3
        if n_dups:
            raise ValueError('w2l_ngram_lm_build: %d duplicate keys' % n_dups)
        (nk, nv, ncap), (tk, tv, tcap) = self.tables
        self.desc = LmTables(ptr(self.prob), ptr(self.bo), ptr(nk), ptr(nv), ncap, ptr(tk), ptr(tv), tcap, ptr(self.trie_word),
                             len(flat['prob']), flat['vocab'], len(tword))
        self.desc_ref = C.byref(self.desc)
