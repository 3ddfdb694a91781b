"""The references of the MBR / device edit-distance tests (mbr_refs.py) checked on the host -- against the library's host edit
distance, exhaustive enumeration, Decoder.wer / Decoder.cer, decode_repeats and mbr.mbr_select_host --, the planted defects the
shared cases must tell apart, the end-to-end inputs' margins, and everything the feature answers without a device."""
import itertools
import math

import numpy as np
import pytest

from mbr_refs import (COLLIDING, DEFECTS, E2E_HOTWORDS, E2E_K, E2E_LEXICON, E2E_N, E2E_SEEDS, ENGLISH, SMALL, brute_alignments,
                      cases, decode_ref, e2e_posteriors, e2e_transitions, edit_ops, mbr_select_ref, nbest_ref, risk_margin_ok,
                      text_tokens, word_hash)
from wav2letter_pytorch_amd import _lib, mbr
from wav2letter_pytorch_amd.decoder import Decoder, _edit_distance

STRINGS = ['', ' ', 'A', 'THE CAT', 'THE  CAT', ' THE CAT ', '  ', 'A B  C   D', "IT'S", 'THE\tCAT\nSAT', 'CAT CBC']


def test_distance_equals_the_host_routine():
    rng = np.random.RandomState(0)
    for trial in range(300):
        alphabet = (2, 4, 1000)[trial % 3]
        a = rng.randint(0, alphabet, size=rng.randint(0, 40))
        b = rng.randint(0, alphabet, size=rng.randint(0, 40))
        assert edit_ops(a, b)[0] == _edit_distance(a, b), (a, b)


def test_brute_force_up_to_length_4():
    for na, nb in itertools.product(range(5), repeat=2):
        for a in itertools.product((0, 1), repeat=na):
            for b in itertools.product((0, 1), repeat=nb):
                every = brute_alignments(a, b)
                got = edit_ops(a, b)
                assert got[0] == min(d for d, _, _, _ in every), (a, b)
                assert got in every, (a, b, got)


def test_identities():
    rng = np.random.RandomState(1)
    for _ in range(200):
        a = rng.randint(0, 3, size=rng.randint(0, 30))
        b = rng.randint(0, 3, size=rng.randint(0, 30))
        d, s, dl, n = edit_ops(a, b)
        assert s + dl + n == d and len(a) - dl + n == len(b) and min(s, dl, n) >= 0
    assert edit_ops([1, 2, 3], []) == (3, 0, 3, 0) and edit_ops([], [1, 2]) == (2, 0, 0, 2) and edit_ops([], []) == (0, 0, 0, 0)


def test_tokenisers_are_the_decoders_views():
    dec = Decoder(ENGLISH)
    for s in STRINGS:
        assert text_tokens(s, 'word') == s.split() == mbr.words_of(s)
        assert text_tokens(s, 'char') == list(s.replace(' ', '')) == mbr.chars_of(s)
    for s1, s2 in itertools.product(STRINGS, repeat=2):
        assert edit_ops(text_tokens(s1, 'word'), text_tokens(s2, 'word'))[0] == dec.wer(s1, s2)
        assert edit_ops(text_tokens(s1, 'char'), text_tokens(s2, 'char'))[0] == dec.cer(s1, s2)
    cls = mbr.label_classes(ENGLISH)
    assert cls[28] == 28 | 0x100 | 0x200 and cls[5] == 5
    assert mbr.label_classes(['a', 'b', 'a', '\t'])[2:].tolist() == [0, 3 | 0x200]


def test_asg_decoding_is_decode_repeats():
    from wav2letter_pytorch_amd.asg import decode_repeats
    rng = np.random.RandomState(2)
    for _ in range(200):
        row = rng.randint(0, 4, size=rng.randint(0, 20)).tolist()
        assert decode_ref(row, 0) == decode_repeats(row, 0) and decode_ref(row, -1) == row
    assert decode_ref([0, 0, 2, 0, 0, 3], 0) == [2, 2, 2, 3]


def test_the_colliding_words_collide():
    a, b = ([ENGLISH.index(ch) for ch in w] for w in COLLIDING)
    assert a != b and len(a) == len(b) and word_hash(a) == word_hash(b)


def _close(a, b):
    return np.allclose(a, b, rtol=1e-12, atol=0, equal_nan=True)


def test_select_ref_against_select_host():
    rows = [('x y', math.log(0.40)), ('a b', math.log(0.35)), ('a c', math.log(0.25))]
    pick, risks, dist = mbr.mbr_select_host(rows, 'word', 1.0)
    assert pick == 1 and dist.tolist() == [[0, 2, 2], [2, 0, 1], [2, 1, 0]]                  # not rank 0
    assert np.allclose(risks, [1.20, 1.05, 1.15], rtol=1e-12)
    ref = mbr_select_ref([text_tokens(s, 'word') for s, _ in rows], [w for _, w in rows])
    assert ref[0] == 1 and _close(ref[1], risks) and (ref[2] == dist).all()
    tie = [('a b', -2.0), ('a c', -2.0), ('d b', -2.0), ('d c', -2.0)]                        # equal weights, k a power of two
    pick, risks, dist = mbr.mbr_select_host(tie, 'word')
    assert pick == 0 and risks.tolist() == [1.0, 1.0, 1.0, 1.0]                               # exact: p_j = 1/4
    assert mbr_select_ref([s.split() for s, _ in tie], [-2.0] * 4)[0] == 0
    rng = np.random.RandomState(3)
    words = ['a', 'b', 'cc', 'd']
    for trial in range(30):
        k = rng.randint(1, 9)
        rows = [(' '.join(words[i] for i in rng.randint(0, 4, size=rng.randint(0, 6))), -float(r) * rng.uniform(0, 2))
                for r in range(k)]
        for unit in ('word', 'char'):
            scale = (1.0, 0.5, 3.0)[trial % 3]
            got = mbr.mbr_select_host(rows, unit, scale)
            ref = mbr_select_ref([text_tokens(s, unit) for s, _ in rows], [w for _, w in rows], scale)
            assert got[0] == ref[0] and _close(got[1], ref[1]) and (got[2] == ref[2]).all(), (rows, unit)


def _outputs(defect):
    """every integer output and pick of the references on cases()"""
    out = []
    for case in cases():
        if case['kind'] == 'pairs':
            if len(case['pairs']) > 600:                # (the 5 000 short pairs: a tenth of them says as much)
                case = dict(case, pairs=case['pairs'][::10])
            out.append([edit_ops(case['seqs'][a], case['seqs'][b], defect) for a, b in case['pairs']
                        if len(case['seqs'][a]) * len(case['seqs'][b]) <= 5000])     # (the long ones are the device's to show)
        else:
            for unit in case['units']:
                ref = nbest_ref(case, unit, defect)
                out.append((ref['pick'].tolist(), ref['status'].tolist(), ref['dist'].tolist(), ref['pick_len'].tolist()))
    return out


@pytest.fixture(scope='module')
def clean_outputs():
    return _outputs(None)


@pytest.mark.parametrize('defect', DEFECTS)
def test_planted_defects_change_an_output(defect, clean_outputs):
    assert _outputs(defect) != clean_outputs


def test_direct_cases_have_no_near_ties_and_cover_the_edges(clean_outputs):
    kinds = set()
    for case in cases():
        if case['kind'] != 'nbest':
            continue
        for unit in case['units']:
            ref = nbest_ref(case, unit)
            for u in range(case['n']):
                assert risk_margin_ok(ref['risk'][u], case['k']), (case['name'], unit, u, ref['risk'][u])
                kinds.add('status1' if ref['status'][u] else 'empty' if (case['len'][u] < 0).all() else
                          'not-rank-0' if ref['pick'][u] else 'rank-0')
    assert kinds == {'status1', 'empty', 'not-rank-0', 'rank-0'}


# ---------------------------------------------------------------------------------------------------- the end-to-end inputs
def _host_nbest(p, **kw):
    """the host search's final beam with its log weights, as the device returns it with nbest = k"""
    from wav2letter_pytorch_amd.beam_search import prefix_beam_search
    stats = {}
    prefix_beam_search(p.astype(np.float64), SMALL, 0, None, E2E_K, stats=stats, **kw)
    beam, w = stats['beam'], stats['weights']
    if kw.get('lexicon') is not None:
        keep = [i for i, s in enumerate(beam) if kw['lexicon'].complete(s, '>')] or list(range(len(beam)))
        beam, w = [beam[i] for i in keep], [w[i] for i in keep]
    return [(s, math.log(x)) for s, x in zip(beam, w) if x > 0]


def test_end_to_end_inputs_move_a_pick_and_have_margins():
    from wav2letter_pytorch_amd.asg_beam import asg_prefix_beam_search
    from wav2letter_pytorch_amd.lexicon import Lexicon
    variants = (('plain', {}), ('lexicon', dict(lexicon=Lexicon(E2E_LEXICON))),
                ('hotwords', dict(hotwords=E2E_HOTWORDS, hotword_weight=1.0)))
    moved = {}
    for seed in E2E_SEEDS:
        p, x = e2e_posteriors(seed), e2e_posteriors(seed, asg=True).astype(np.float64)
        g = e2e_transitions(seed).astype(np.float64)
        lists = {name: [_host_nbest(p[u], **kw) for u in range(E2E_N)] for name, kw in variants}
        lists['asg'] = [asg_prefix_beam_search(x[u], g, SMALL, k=E2E_K, nbest=E2E_K, return_weights=True) for u in range(E2E_N)]
        for name, per_utt in lists.items():
            for unit in ('word', 'char'):
                for u, rows in enumerate(per_utt):
                    pick, risk, _ = mbr_select_ref([text_tokens(s, unit) for s, _ in rows], [w for _, w in rows])
                    assert risk_margin_ok(risk, E2E_K), (seed, name, unit, u, risk)
                    moved[name] = moved.get(name, False) or pick != 0
    assert moved['plain'] and moved['asg'], moved



# ------------------------------------------------------------------------------------------------------------ host answers
def test_workspace_queries():
    lib = _lib.lib
    assert lib.w2l_edit_distance_workspace_bytes(100, 4, 2, 4095) == 0
    assert lib.w2l_edit_distance_workspace_bytes(100, 4, 2, 4096) == -1
    for bad in ((-1, 4, 2, 10), (1 << 31, 4, 2, 10), (100, 0, 2, 10), (100, 4, 0, 10), (100, 4, 2, -1)):
        assert lib.w2l_edit_distance_workspace_bytes(*bad) == -1
    assert lib.w2l_nbest_mbr_workspace_bytes(3, 8, 40) == (4 * 3 * 8 * 40 + 3 * 8) * 4
    for bad in ((0, 8, 40), (3, 0, 40), (3, 65, 40), (3, 8, 0), (3, 8, 32769), (65536, 8, 40)):
        assert lib.w2l_nbest_mbr_workspace_bytes(*bad) == -1
    assert lib.w2l_abi_version() == 2
    assert _lib.TRACE_NAMES['w2l_edit_distance'] and _lib.TRACE_NAMES['w2l_nbest_mbr']


def test_section_layout():
    o = mbr.mbr_sections(3, 8, 40)
    assert o == (0, 12, 24, 24 + 8 * 24, 216 + 4 * 192, 984 + 12, 996 + 480) and o.risk % 8 == 0
    assert [mbr.mbr_offset(b) for b in (0, 4, 8, 12)] == [0, 8, 8, 16]


def test_python_validation_needs_no_device():
    from wav2letter_pytorch_amd.asg_beam import ASGBeamSearchDecoder, asg_beam_search_gpu
    from wav2letter_pytorch_amd.beam_search import GPUPrefixBeamSearchDecoder, prefix_beam_search_gpu
    p = np.full((4, 6), 1 / 6, dtype=np.float32)
    for search, head in ((prefix_beam_search_gpu, (p, SMALL)), (asg_beam_search_gpu, (np.log(p), None, SMALL))):
        with pytest.raises(ValueError, match="'word', 'char'"):
            search(*head, mbr='sentence')
        for scale in (float('nan'), float('inf'), -1.0):
            with pytest.raises(ValueError, match='mbr_scale'):
                search(*head, mbr='word', mbr_scale=scale)
        with pytest.raises(ValueError, match='return_risks'):
            search(*head, return_risks=True)
    with pytest.raises(ValueError, match="'word', 'char'"):
        GPUPrefixBeamSearchDecoder(None, SMALL, mbr='words')
    with pytest.raises(ValueError, match='mbr_scale'):
        ASGBeamSearchDecoder(SMALL, mbr='char', mbr_scale=-2)
    dec = GPUPrefixBeamSearchDecoder(None, SMALL, mbr='char', mbr_scale=2)
    assert (dec.mbr, dec.mbr_scale) == ('char', 2.0) and GPUPrefixBeamSearchDecoder(None, SMALL).mbr is None
    with pytest.raises(ValueError, match='4095'):
        mbr.edit_distance_gpu([list(range(4096))], [[1]])
    with pytest.raises(ValueError, match='4095'):
        mbr.edit_distance_gpu(['a ' * 4096], ['a'])
    with pytest.raises(ValueError, match='unit'):
        mbr.edit_distance_gpu(['a'], ['a'], unit='line')
    with pytest.raises(ValueError, match='references'):
        mbr.edit_distance_gpu(['a', 'b'], ['a'])
    with pytest.raises(ValueError, match='outside'):
        mbr.edit_distance_pairs_gpu([[1], [2]], [(0, 2)])
    assert mbr.edit_distance_gpu([], []).shape == (0,) and mbr.edit_distance_gpu([], [], counts=True)[1].shape == (0, 3)
    with pytest.raises(ValueError, match='no rows'):
        mbr.mbr_select_host([], 'word')


def test_command_line_rules():
    from wav2letter_pytorch_amd import test as T
    base = ['model_path=a.ckpt', 'data.test_manifest=m.csv']
    asg = base + ['model.criterion=asg']
    for dec, name in ((base + ['decoder=beam'], 'GPUPrefixBeamSearchDecoder'),
                      (base + ['decoder=beam_lm', 'lm_path=lm.arpa'], 'GPUPrefixBeamSearchLMDecoder'),
                      (asg + ['decoder=asg_beam'], 'ASGBeamSearchDecoder'),
                      (asg + ['decoder=asg_beam_lm', 'lm_path=lm.arpa'], 'ASGBeamSearchLMDecoder')):
        plain = T.decoder_spec(T.build_config(dec), True)
        assert plain[0] == name and 'mbr' not in plain[1] and 'mbr_scale' not in plain[1]     # today's dictionaries
        got = T.decoder_spec(T.build_config(dec + ['mbr=word']), True)
        assert got == (name, dict(plain[1], mbr='word'))
        got = T.decoder_spec(T.build_config(dec + ['mbr=char', 'mbr_scale=0.5']), True)
        assert got == (name, dict(plain[1], mbr='char', mbr_scale=0.5))
    for argv in (base + ['mbr=word'], base + ['decoder=greedy', 'mbr=char']):
        with pytest.raises(SystemExit, match='mbr is given but decoder=greedy'):
            T.build_config(argv)
    with pytest.raises(SystemExit, match='mbr_scale is given without mbr'):
        T.build_config(base + ['decoder=beam', 'mbr_scale=2'])
    with pytest.raises(SystemExit, match="mbr='sentence'"):
        T.build_config(base + ['decoder=beam', 'mbr=sentence'])
    for bad in ('much', 'inf', '-1'):
        with pytest.raises(SystemExit, match='mbr_scale'):
            T.build_config(base + ['decoder=beam', 'mbr=word', 'mbr_scale=' + bad])
    with pytest.raises(SystemExit) as err:                # not a beam.* option
        T.build_config(base + ['decoder=beam', 'beam.mbr=word'])
    assert str(err.value) == "unknown beam option(s) ['mbr']: beam.k, beam.alpha, beam.beta, beam.prune"
    assert T.build_config(base + ['error_counts=true']).error_counts is True and T.build_config(base).error_counts is False
    assert T.BEAM_DEFAULTS == dict(k=5, alpha=0.3, beta=5, prune=1e-3)


def test_decoders_pass_mbr_on_only_when_set(monkeypatch):
    from wav2letter_pytorch_amd import asg_beam, beam_search
    seen = []
    monkeypatch.setattr(beam_search, 'prefix_beam_search_gpu', lambda *a, **kw: seen.append(kw) or ['x'])
    monkeypatch.setattr(asg_beam, 'asg_beam_search_gpu', lambda *a, **kw: seen.append(kw) or ['x'])
    p = np.zeros((1, 4, 6), dtype=np.float32)
    beam_search.GPUPrefixBeamSearchDecoder(None, SMALL).decode(p)
    beam_search.GPUPrefixBeamSearchDecoder(None, SMALL, mbr='word').decode(p)
    asg_beam.ASGBeamSearchDecoder(SMALL).decode(p)
    asg_beam.ASGBeamSearchDecoder(SMALL, mbr='char', mbr_scale=0.25).decode(p)
    assert 'mbr' not in seen[0] and 'mbr' not in seen[2]
    assert (seen[1]['mbr'], seen[1]['mbr_scale']) == ('word', 1.0) and (seen[3]['mbr'], seen[3]['mbr_scale']) == ('char', 0.25)
