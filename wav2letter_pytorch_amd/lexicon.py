"""A word list that constrains the CTC prefix beam searches (beam_search.prefix_beam_search, prefix_beam_search_gpu): no mass
is ever given to a string that leaves the lexicon.

Definition, shared by the host recursion and the device kernels.  A *separator* is the space or ``end_char``.  The *partial
word* of a string is what follows its last separator (the whole string if it has none).  A string is **legal** when

  * every separator in it closes an empty partial word or a lexicon word (doubled and leading spaces are legal), and
  * its trailing partial word is empty or a prefix of a lexicon word.

Legal strings are prefix-closed.  A legal string is **complete** when its trailing partial word is empty or a whole word.
``Lexicon.allows`` / ``Lexicon.complete`` state this with ``str`` operations and are the oracle of everything else.

Device layout (``spelling_trie`` / ``to_device``): the flat trie of ngram_lm.ArpaLM.spelling_trie -- an open-addressing table
keyed by the exact pair (trie node << 8 | canonical label) -> child node, root 0, and ``word[node] >= 0`` where a node spells a
whole word -- so the trie of an n-gram model is a lexicon as it is (``Lexicon.from_lm`` shares it, see ``to_device``).

The same container holds a list of **hotwords** (``hotwords=`` of the searches): there the walk over the trie removes nothing,
it counts the characters ``h`` that the search rewards (``Lexicon.boost_chars``, the oracle of that feature)."""
from __future__ import annotations

import ctypes as C
import gzip
import os
from typing import Dict, Iterable, List, Sequence

import numpy as np

from .ngram_lm import build_spelling_trie, table_capacity

_LM_SPECIALS = ('<unk>', '<s>', '</s>')


def _read_words(path) -> Iterable[str]:
    with open(path, 'rb') as f:
        gz = f.read(2) == b'\x1f\x8b'
    with (gzip.open(path, 'rt', encoding='utf-8') if gz else open(path, 'r', encoding='utf-8')) as f:
        for line in f:
            fields = line.split()
            if fields and not fields[0].startswith('#'):
                yield fields[0]                        # flashlight style: word, then its spelling


class Lexicon:
    """``source``: a path (plain or gzip; one entry per line, the word is the first whitespace-separated token, empty lines
    and lines starting with ``#`` are skipped) or an iterable of words.  ``words`` keeps the first occurrence of each word in
    order; ``stats['duplicates']`` counts the others."""

    def __init__(self, source):
        if isinstance(source, (str, os.PathLike)):
            self.path = str(source)
            given = _read_words(source)
        else:
            self.path = None
            given = source
        self.words: List[str] = []
        seen = set()
        dups = 0
        for w in given:
            if not isinstance(w, str) or not w or any(ch.isspace() for ch in w):
                raise ValueError('Lexicon: %r is not a word (a non-empty string without whitespace)' % (w,))
            if w in seen:
                dups += 1
                continue
            seen.add(w)
            self.words.append(w)
        self._words = frozenset(seen)
        self._prefixes = frozenset(w[:i] for w in self.words for i in range(len(w) + 1))
        self.stats = dict(words=len(self.words), duplicates=dups, unspellable=0)
        self.lm = None                                 # from_lm: the model whose vocabulary this is
        self._tries: Dict[tuple, tuple] = {}
        self._spellable: Dict[tuple, 'Lexicon'] = {}
        self._device: Dict[tuple, 'DeviceLexicon'] = {}

    @classmethod
    def from_lm(cls, arpa) -> 'Lexicon':
        """the vocabulary of an ngram_lm.ArpaLM without <unk>, <s>, </s>"""
        lex = cls(w for w in arpa.words if w not in _LM_SPECIALS)
        lex.lm = arpa
        return lex

    def __len__(self):
        return len(self.words)

    def __contains__(self, word):
        return word in self._words

    # ------------------------------------------------------------------------------------------------------- the definition
    @staticmethod
    def _parts(string: str, end_char: str) -> List[str]:
        """the closed partial words of ``string`` and, last, its trailing partial word"""
        if end_char:
            string = string.replace(end_char, ' ')
        return string.split(' ')

    def allows(self, string: str, end_char: str = '>') -> bool:
        """``string`` is legal"""
        parts = self._parts(string, end_char)
        return all(p == '' or p in self._words for p in parts[:-1]) and parts[-1] in self._prefixes

    def complete(self, string: str, end_char: str = '>') -> bool:
        """the trailing partial word of ``string`` is empty or a whole lexicon word"""
        last = self._parts(string, end_char)[-1]
        return last == '' or last in self._words

    def boost_chars(self, string: str, end_char: str = '>') -> int:
        """``h(string)`` of hotword boosting, this list being the hotwords: the characters of the closed words (those followed
        by a separator) that are in the list, plus the characters of the trailing partial word if it is non-empty and a prefix
        of a word of the list (a whole word counts).  The partial word's credit is provisional: it is gone when the word
        leaves the list's prefixes or is closed as something that is not in the list."""
        parts = self._parts(string, end_char)
        h = sum(len(p) for p in parts[:-1] if p in self._words)
        if parts[-1] and parts[-1] in self._prefixes:
            h += len(parts[-1])
        return h

    def spellable(self, labels: Sequence[str], blank_index: int = 0) -> 'Lexicon':
        """the Lexicon of the words that ``labels`` can spell (spelling_trie's rule; this one if it drops none), so that the
        ``str`` oracle speaks of the words the flat trie holds.  ValueError if none is left."""
        labels = list(labels)
        ck = (tuple(labels), blank_index)
        if ck not in self._spellable:
            ok = set(labels) - {labels[blank_index]}
            kept = [w for w in self.words if all(ch in ok for ch in w)]
            self.stats['unspellable'] = len(self.words) - len(kept)
            if not kept:
                raise ValueError('Lexicon: none of the %d words can be spelled with the labels %r' % (len(self.words),
                                                                                                   ''.join(labels)))
            self._spellable[ck] = self if len(kept) == len(self.words) else Lexicon(kept)
        return self._spellable[ck]

    # ---------------------------------------------------------------------------------------------------------- flat trie
    def spelling_trie(self, labels: Sequence[str], blank_index: int = 0):
        """(keys uint64 (node << 8 | canonical label), vals int32 (child node), word int32 [nodes] (index into ``words``, -1))
        of the words that ``labels`` can spell: every character a label other than the blank's; a duplicate label spells with
        its first index.  The others are counted in ``stats['unspellable']``; ValueError if none is left."""
        labels = list(labels)
        ck = (tuple(labels), blank_index)
        if ck not in self._tries:
            keys, vals, word, dropped = build_spelling_trie(enumerate(self.words), labels, blank_index)
            self.stats['unspellable'] = dropped
            if dropped == len(self.words):
                raise ValueError('Lexicon: none of the %d words can be spelled with the labels %r' % (len(self.words),
                                                                                                   ''.join(labels)))
            self._tries[ck] = (keys, vals, word)
        return self._tries[ck]

    def shares_trie_with_lm(self, labels: Sequence[str], blank_index: int = 0) -> bool:
        """from_lm only: the model's own spelling trie has the nodes and whole-word marks of this lexicon's (it has unless
        the labels can spell <unk>, <s> or </s>), so the model's device tables serve as the lexicon's"""
        if self.lm is None:
            return False
        mine, theirs = self.spelling_trie(labels, blank_index), self.lm.spelling_trie(labels, blank_index)
        return (np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
                and np.array_equal(mine[2] >= 0, theirs[2] >= 0))

    def to_device(self, labels: Sequence[str], blank_index: int = 0, device=None) -> 'DeviceLexicon':
        """the trie's hash table built on the device by w2l_ngram_lm_build; cached per (labels, blank, device).  A from_lm
        lexicon whose trie is the model's (shares_trie_with_lm) points at the model's device tables: nothing is uploaded twice."""
        import torch
        dev = torch.device(device if device is not None else 'cuda')
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        ck = (tuple(labels), blank_index, str(dev))
        if ck not in self._device:
            self._device[ck] = DeviceLexicon(self, list(labels), blank_index, dev)
        return self._device[ck]


class DeviceLexicon:
    """device tensors of one Lexicon for one label set (w2l_lexicon_t); ``shared``: they are the language model's"""

    def __init__(self, lex: Lexicon, labels, blank_index, dev):
        import torch
        from ._lib import LexTables, check, lib, ptr, stream_ptr
        self.shared = lex.shares_trie_with_lm(labels, blank_index)
        if self.shared:
            self.owner = lex.lm.to_device(labels, blank_index, dev)        # keeps the tables alive
            self.trie_keys, self.trie_vals, self.trie_cap = self.owner.tables[1]
            self.trie_word = self.owner.trie_word
        else:
            keys, vals, word = lex.spelling_trie(labels, blank_index)
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
            self.trie_word = to(word)
            self.trie_cap = table_capacity(len(keys))
            self.trie_keys = torch.empty(self.trie_cap, dtype=torch.int64, device=dev)
            self.trie_vals = torch.empty(self.trie_cap, dtype=torch.int32, device=dev)
            dups = torch.zeros(1, dtype=torch.int32, device=dev)
            k_dev, v_dev = to(keys.view(np.int64)), to(vals)
            check(lib.w2l_ngram_lm_build(ptr(k_dev), ptr(v_dev), len(keys), ptr(self.trie_keys), ptr(self.trie_vals),
                                         self.trie_cap, ptr(dups), stream_ptr()), 'w2l_ngram_lm_build')
            if int(dups.item()):                       # (synchronises: k_dev / v_dev may go)
                raise ValueError('w2l_ngram_lm_build: %d duplicate keys' % int(dups.item()))
        self.desc = LexTables(ptr(self.trie_keys), ptr(self.trie_vals), self.trie_cap, ptr(self.trie_word),
                              int(self.trie_word.numel()))
        self.desc_ref = C.byref(self.desc)
