"""CTC keyword search on a real MI355X: w2l_ctc_kws (csrc/ctc_kws.hip) through keyword_search.ctc_keyword_search against the
float64 references of tests/kws_refs.py -- the curves within the fp32 bound derived there, the start frames checked free of
tie-breaking by the forced alignment of the slice they name, the hits against the host pick rule on the device's own curves --
then planted occurrences, the error statuses, table reuse, and find_keywords / the search command line end to end."""
import functools
import json
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kws_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

NINF = float('-inf')
THRESHOLD, MAX_HITS = -3.0, 4          # nats per label: loose enough that random posteriors give hits, overlaps and truncation
LONG_KW = list(range(1, 29)) * 9 + [1, 2, 3]           # 255 labels: 509 states, alone in a 512-lane block


def _keywords(A, K):
    if K == 1:
        return [[2, 4, 1]]
    g = np.random.default_rng(100 + A)
    kws = [g.integers(1, A, int(s)).tolist() for s in g.integers(1, 9, K)]
    kws[3], kws[11] = [2, 2, 4], [A - 1]               # a doubled letter, a single label
    return kws


@functools.lru_cache(maxsize=None)
def _case(A, T, K, log_probs, long_kw=False):
    """the shared inputs and float64 references of one shape: x [3, T, A] fp32 (what the device reads), its float64
    log-probabilities, lengths {T, T // 2, 0}, the keywords and per (utterance, keyword) kws_refs.scan_ref"""
    lp = np.stack([R.random_lp(1000 * A + 10 * T + n, T, A, 0.1 if A == 6 else 0.0) for n in range(3)])
    if log_probs:
        x, lp64 = lp, lp.astype(np.float64)
    else:
        x = np.exp(lp.astype(np.float64)).astype(np.float32)
        with np.errstate(divide='ignore'):
            lp64 = np.log(x.astype(np.float64))
    lengths = [T, T // 2, 0]
    kws = [LONG_KW] if long_kw else _keywords(A, K)
    refs = [[R.scan_ref(lp64[n], kw, length=lengths[n]) for kw in kws] for n in range(3)]
    for rows in refs:
        for r in rows:
            r['end_score'].setflags(write=False)
            r['end_start'].setflags(write=False)
    return dict(x=x, lp64=lp64, lengths=lengths, kws=kws, refs=refs)


def _expected_hits(score, start, table_lengths, threshold, max_hits):
    """pick_hits_host on curves [N, K, T] -> ctc_keyword_search's format"""
    from wav2letter_pytorch_amd.keyword_search import pick_hits_host
    out = []
    for n in range(score.shape[0]):
        hits = []
        for k in range(score.shape[1]):
            thr = np.float32(threshold) * np.float32(table_lengths[k])
            hits += [(k, s, e, float(np.float32(v))) for s, e, v in pick_hits_host(score[n, k], start[n, k], thr, max_hits)]
        out.append(sorted(hits, key=lambda h: (h[1], h[2], h[0])))
    return out


def _check_against_refs(c, found, score, start, log_probs):
    """checks 1 to 3 of one case -> the number of hits"""
    worst = 0.0
    for n, Tn in enumerate(c['lengths']):
        for k, kw in enumerate(c['kws']):
            ref = c['refs'][n][k]
            got, st = score[n, k], start[n, k]
            finite = ref['end_score'] > NINF
            assert np.array_equal(got > NINF, finite), (n, k)                   # -inf exactly where the reference has it
            assert (st[~finite] == -1).all() and not np.isnan(got).any()
            bound = R.kws_bound(Tn, ref['P'])
            if finite.any():
                err = np.abs(got[finite].astype(np.float64) - ref['end_score'][finite]).max()
                worst = max(worst, err / bound if bound else (0.0 if err == 0 else np.inf))
                assert err <= bound, (n, k, err, bound)
            # starts, free of tie-breaking: the keyword aligns within [end_start[t], t] with the score the device reports
            for t in np.nonzero(finite)[0]:
                assert 0 <= st[t] <= t < Tn
                sl = R.slice_score(c['lp64'][n], kw, int(st[t]), int(t))
                assert sl > NINF and abs(sl - float(got[t])) <= bound, (n, k, t, sl, got[t], bound)
            assert (got <= 0).all()
    print(f'log_probs={log_probs}: worst curve error {worst:.3f} of the bound')
    want = _expected_hits(score, start, [len(kw) for kw in c['kws']], THRESHOLD, MAX_HITS)
    assert found == want
    assert found[2] == []                                                       # the utterance of no frames
    return sum(len(f) for f in found)


@pytest.mark.parametrize('log_probs', [True, False])
@pytest.mark.parametrize('K', [1, 40])
@pytest.mark.parametrize('T', [1, 17, 100])
@pytest.mark.parametrize('A', [6, 29])
def test_curves_starts_and_hits_against_float64(A, T, K, log_probs):
    from wav2letter_pytorch_amd.keyword_search import KeywordTable, ctc_keyword_search
    c = _case(A, T, K, log_probs)
    table = KeywordTable(c['kws'])
    if K == 40:
        assert table.chunks[0]['width'] == 64 and table.chunks[0]['n_blocks'] >= 2
        assert (np.diff(table.chunks[0]['block_kw']) >= 2).any()                # several keywords share a block
    found, score, start = ctc_keyword_search(torch.from_numpy(c['x']).cuda(), table, input_lengths=c['lengths'], log_probs=log_probs,
                                             threshold=THRESHOLD, max_hits=MAX_HITS, return_curves=True)
    assert score.shape == start.shape == (3, K, T) and score.dtype == np.float32 and start.dtype == np.int32
    hits = _check_against_refs(c, found, score, start, log_probs)
    if T == 100 and K == 40:
        assert hits > 0
        per_kw = {}
        for k, s, e, v in found[0]:
            per_kw[k] = per_kw.get(k, 0) + 1
        assert max(per_kw.values()) == MAX_HITS                                 # the truncation is exercised


@pytest.mark.parametrize('log_probs', [True, False])
def test_a_keyword_of_255_labels_alone_in_the_widest_block(log_probs):
    from wav2letter_pytorch_amd.keyword_search import KeywordTable, ctc_keyword_search
    c = _case(29, 300, 1, log_probs, long_kw=True)
    table = KeywordTable(c['kws'])
    assert table.chunks[0]['width'] == 512 and table.chunks[0]['n_blocks'] == 1
    found, score, start = ctc_keyword_search(torch.from_numpy(c['x']).cuda(), table, input_lengths=c['lengths'], log_probs=log_probs,
                                             threshold=THRESHOLD, max_hits=MAX_HITS, return_curves=True)
    assert (score[0, 0, 254:] > NINF).all() and (score[0, 0, :254] == NINF).all() and (score[1:] == NINF).all()
    _check_against_refs(c, found, score, start, log_probs)


def test_every_block_width_gives_the_same_curves():
    from wav2letter_pytorch_amd.keyword_search import WIDTHS, KeywordTable, ctc_keyword_search
    c = _case(29, 17, 40, True)
    x = torch.from_numpy(c['x']).cuda()
    base = None
    for w in WIDTHS:
        got = ctc_keyword_search(x, KeywordTable(c['kws'], width=w), input_lengths=c['lengths'], log_probs=True, threshold=THRESHOLD,
                                 max_hits=MAX_HITS, return_curves=True)
        if base is None:
            base = got
        assert got[0] == base[0] and np.array_equal(got[1].view(np.uint32), base[1].view(np.uint32)) and np.array_equal(got[2], base[2]), w


@pytest.mark.parametrize('log_probs', [True, False])
def test_planted_occurrences_are_found_exactly(log_probs):
    from wav2letter_pytorch_amd.keyword_search import ctc_keyword_search
    lp = R.planted_lp(21, 32, 6, R.path_of(R.PLANTED_SPANS))
    x = lp if log_probs else np.exp(lp.astype(np.float64)).astype(np.float32)
    for t, a in R.path_of(R.PLANTED_SPANS).items():
        assert x[t].argmax() == a and (x[t] == x[t, a]).sum() == 1
    other = R.random_lp(5, 32, 6)
    batch = np.stack([x, other if log_probs else np.exp(other), x])
    found, score, start = ctc_keyword_search(batch, [R.PLANTED_KW, [5, 5]], input_lengths=[32, 32, 20], log_probs=log_probs,
                                             return_curves=True)
    mine = [h for h in found[0] if h[0] == 0]
    assert [(h[1], h[2]) for h in mine] == R.PLANTED_SEGMENTS and all(h[3] == 0.0 for h in mine)
    for (s, e), last in zip(R.PLANTED_SEGMENTS, ([11, 12, 13], [25, 26, 27])):
        assert (score[0, 0, last] == 0).all() and (start[0, 0, last] == s).all()
    assert [(h[1], h[2]) for h in found[2] if h[0] == 0] == R.PLANTED_SEGMENTS[:1]          # 20 frames: the first occurrence only
    assert (score[2, :, 20:] == NINF).all() and (start[2, :, 20:] == -1).all()


def _raw(x, lengths, table, threshold, max_hits, log_probs, blank=0):
    """one w2l_ctc_kws call below ctc_keyword_search's status check -> (status, count, hits, score, start) on the host"""
    from wav2letter_pytorch_amd.keyword_search import HIT_DTYPE, kws_sections, launch_kws
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n, t, _ = x.shape
    k = len(table)
    _, dev_table = table.on_device(0, xd.device)
    thr = torch.from_numpy(np.float32(threshold) * table.lengths.astype(np.float32)).cuda()
    o = kws_sections(n, k, max_hits)
    small = torch.full((o[3],), 0x5A, dtype=torch.uint8, device='cuda')
    score = torch.full((n, k, t), 7.0, device='cuda')
    start = torch.full((n, k, t), 7, dtype=torch.int32, device='cuda')
    sz = torch.tensor(lengths, dtype=torch.int32).cuda() if lengths is not None else None
    launch_kws(xd, sz, dev_table, thr, max_hits, blank, log_probs, small, score, start)
    host = small.cpu().numpy()
    return (host[o[0]:o[1]].view(np.int32), host[o[1]:o[2]].view(np.int32).reshape(n, k),
            host[o[2]:o[3]].view(HIT_DTYPE).reshape(n, k, max_hits), score.cpu().numpy(), start.cpu().numpy())


def test_bad_frames_and_bad_labels_give_status_2():
    """A frame of all -inf, a NaN or a negative probability: status 2 for that utterance only.  A bad label sits in the table,
    which every utterance shares: status 2 for every utterance, and the keywords of the other blocks keep their curves."""
    from wav2letter_pytorch_amd.keyword_search import KeywordTable, ctc_keyword_search
    c = _case(6, 17, 40, True)
    table = KeywordTable(c['kws'])
    lengths = [17, 8, 17]
    clean = _raw(c['x'], lengths, table, THRESHOLD, MAX_HITS, True)
    assert clean[0].tolist() == [0, 0, 0]
    for mode, value, log_probs in (('ninf', NINF, True), ('nan', np.nan, True), ('neg', -0.25, False), ('zero', 0.0, False)):
        x = c['x'].copy() if log_probs else np.exp(c['x'].astype(np.float64)).astype(np.float32)
        base = clean if log_probs else _raw(x, lengths, table, THRESHOLD, MAX_HITS, False)
        x[1, 12] = value                                 # past utterance 1's 8 frames: not read
        same = _raw(x, lengths, table, THRESHOLD, MAX_HITS, log_probs)
        assert same[0].tolist() == [0, 0, 0] and all(np.array_equal(a, b) for a, b in zip(same[1:], base[1:])), mode
        if mode in ('ninf', 'zero'):
            x[1, 3] = value                              # the whole frame: no finite maximum
        else:
            x[1, 3, 2] = value                           # one entry
        got = _raw(x, lengths, table, THRESHOLD, MAX_HITS, log_probs)
        assert got[0].tolist() == [0, 2, 0], mode
        for part, ref in zip(got[1:], base[1:]):         # the others are unaffected
            assert np.array_equal(part[[0, 2]], ref[[0, 2]]), mode
        assert (got[1][1] == 0).all() and (got[3][1] == NINF).all() and (got[4][1] == -1).all()
        with pytest.raises(ValueError, match=r'utterances \[1\]'):
            ctc_keyword_search(x, table, input_lengths=lengths, log_probs=log_probs)
    # a label out of range, and the blank, on a label state of keyword 5 (a crafted table: the host refuses both before a launch)
    chunk = table.chunks[0]
    lane = int(np.nonzero((chunk['meta'] >> 4 == 5) & (chunk['meta'] >= 0))[0][0])
    blk = lane // chunk['width']
    others = [k for k in range(40) if not chunk['block_kw'][blk] <= k < chunk['block_kw'][blk + 1]]
    assert others and (chunk['meta'][lane] & 8)
    for bad_label in (6, -1, 0, 1 << 30):
        crafted = KeywordTable(c['kws'])
        buf, _ = crafted.on_device(0, torch.device('cuda', torch.cuda.current_device()))
        buf[lane] = bad_label
        got = _raw(c['x'], lengths, crafted, THRESHOLD, MAX_HITS, True)
        assert got[0].tolist() == [2, 2, 2], bad_label
        assert np.array_equal(got[3][:, others], clean[3][:, others]) and np.array_equal(got[4][:, others], clean[4][:, others])
        assert (got[1] == 0).all()


def test_argument_errors_launch_nothing():
    import ctypes as C
    from wav2letter_pytorch_amd._lib import KwsTable, lib, ptr, stream_ptr
    from wav2letter_pytorch_amd.keyword_search import KeywordTable
    table = KeywordTable([[1, 2], [3]])
    _, good = table.on_device(0, torch.device('cuda', torch.cuda.current_device()))
    x = torch.zeros(2, 5, 4, device='cuda')
    thr = torch.zeros(2, device='cuda')
    out = torch.full((4096,), 7, dtype=torch.uint8, device='cuda')
    ws = torch.empty(int(lib.w2l_ctc_kws_workspace_bytes(2, 5, 2, 8)), dtype=torch.uint8, device='cuda')

    def call(t=good, n=2, T=5, A=4, blank=0, max_hits=8, phases=7, ws_bytes=ws.numel()):
        p = C.c_void_p(out.data_ptr())
        return lib.w2l_ctc_kws(ptr(x), None, n, T, A, blank, 1, C.byref(t), ptr(thr), max_hits, phases, ptr(ws), ws_bytes, p, p, p, p, p,
                               stream_ptr())

    def variant(**kw):
        t = KwsTable.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    for bad in (dict(n=0), dict(T=0), dict(T=32769), dict(A=0), dict(blank=4), dict(blank=-1), dict(max_hits=0), dict(max_hits=65),
                dict(phases=0), dict(phases=8), dict(ws_bytes=ws.numel() - 1), dict(t=variant(width=96)), dict(t=variant(n_blocks=0)),
                dict(t=variant(n_blocks=3)), dict(t=variant(n_keywords=4097)), dict(t=variant(labels=None)), dict(t=variant(meta=None))):
        assert call(**bad) != 0, bad
        assert lib.w2l_last_error().startswith(b'ctc_kws:'), lib.w2l_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all())                        # nothing was launched


def test_a_table_reused_across_batches_equals_a_fresh_one():
    from wav2letter_pytorch_amd.keyword_search import KeywordTable, ctc_keyword_search
    a, b = _case(29, 17, 40, True), _case(29, 100, 40, False)
    table = KeywordTable(a['kws'])
    for c, log_probs in ((a, True), (b, False), (a, True)):
        x = torch.from_numpy(c['x']).cuda()
        kw = dict(input_lengths=c['lengths'], log_probs=log_probs, threshold=THRESHOLD, max_hits=MAX_HITS, return_curves=True)
        got, fresh = ctc_keyword_search(x, table, **kw), ctc_keyword_search(x, KeywordTable(a['kws']), **kw)
        assert got[0] == fresh[0] and np.array_equal(got[1].view(np.uint32), fresh[1].view(np.uint32)) and np.array_equal(got[2], fresh[2])
    assert len(table._device) == 1                       # uploaded once


def test_decoder_find_with_strings():
    from wav2letter_pytorch_amd.decoder import GreedyDecoder
    labels = ['_', 'a', 'b', 'c', ' ', 'd']
    dec = GreedyDecoder(labels)
    spans = [(0, 0, 1), (1, 2, 3), (2, 4, 4), (4, 5, 6), (3, 7, 8), (0, 9, 11)]                  # "ab c"
    lp = R.planted_lp(8, 12, 6, R.path_of(spans))
    found = dec.find(torch.from_numpy(lp).cuda(), ['ab c', 'b c', 'dd'], log_probs=True)
    assert [(k, s, e) for k, s, e, v in found[0] if v == 0.0] == [(0, 2, 8), (1, 4, 8)]
    assert dec.find(np.exp(lp), 'ab c')[0][0][:3] == (0, 2, 8)
    with pytest.raises(ValueError):
        dec.find(lp, ['ax'])


# ---------------------------------------------------------------------------------------------------------------- the model
def _speechlike(seed, bursts, seconds, rate=16000):
    g = np.random.default_rng(seed)
    x = 1e-3 * g.standard_normal(int(seconds * rate))
    for a, b in bursts:
        i, j = int(a * rate), int(b * rate)
        x[i:j] += 0.3 * g.standard_normal(j - i)
    return x.astype(np.float32)


PHRASES = ['the', 'a cat', 'oo']
LOOSE = dict(threshold=-40.0, max_hits=3)                # an untrained model: loose enough that every piece gives hits


@pytest.fixture(scope='module')
def model():
    from wav2letter_pytorch_amd import Wav2Letter
    from wav2letter_pytorch_amd.defaults import wav2letter_model
    torch.manual_seed(7)
    return Wav2Letter(wav2letter_model(mid_layers=1, dropout=False)).cuda().eval()


def _by_hand(model, x, phrases):
    """find_keywords' answer from its parts: the VAD's pieces, each through the front end, infer and ctc_keyword_search"""
    from wav2letter_pytorch_amd.evaluate import frame_seconds
    from wav2letter_pytorch_amd.keyword_search import ctc_keyword_search
    from wav2letter_pytorch_amd.segmentation import vad_segments
    segs = vad_segments([x])[0]
    ext = model._transcribe_extractor
    ratio = frame_seconds(model)
    want = []
    with torch.no_grad():
        for a, b in segs.tolist():
            rows = torch.from_numpy(x[a:b]).cuda().view(1, -1)
            feats, lens = ext.extract_rows(rows, np.array([b - a], dtype=np.int32))
            out, out_lens = model.infer(feats, lens)
            found = ctc_keyword_search(out, phrases, input_lengths=out_lens, labels=list(model.labels), log_probs=True, **LOOSE)[0]
            want += [{'keyword': phrases[k], 'start': a / 16000.0 + float(s * ratio), 'end': a / 16000.0 + float(e * ratio), 'score': v}
                     for k, s, e, v in found]
    return segs, sorted(want, key=lambda h: (h['start'], h['end']))


def test_find_keywords_on_a_recording_of_two_pieces(model, monkeypatch):
    monkeypatch.setattr('wav2letter_pytorch_amd.data.data_loader.SpectrogramExtractor.dithering', 0.0)
    x = _speechlike(1, ((0.5, 1.5), (2.5, 3.3)), 4.0)
    got = model.find_keywords([x], PHRASES, batch_size=1, **LOOSE)[0]
    segs, want = _by_hand(model, x, PHRASES)
    assert len(segs) == 2
    assert got == want and len(got) > 0
    starts = segs[:, 0] / 16000.0
    assert any(h['start'] >= starts[1] for h in got) and any(h['start'] < starts[1] for h in got)        # hits in both pieces
    assert all(h['start'] <= h['end'] and h['score'] <= 0 for h in got)
    both = model.find_keywords(x, PHRASES, batch_size=1, also_transcribe=True, **LOOSE)[0]
    assert both[0] == got and both[1] == model.transcribe_long([x], batch_size=1)[0]
    assert model.find_keywords([np.zeros(32000, dtype=np.float32)], PHRASES) == [[]]
    with pytest.raises(ValueError):
        model.find_keywords([x], ['the', 'café'])


def test_search_command_line(model, tmp_path, monkeypatch):
    from wav2letter_pytorch_amd import search as S
    from wav2letter_pytorch_amd.data.data_loader import read_audio
    monkeypatch.setattr('wav2letter_pytorch_amd.data.data_loader.SpectrogramExtractor.dithering', 0.0)
    paths = []
    for i, bursts in enumerate((((0.5, 1.5), (2.5, 3.3)), ((0.3, 1.0),))):
        sig = _speechlike(20 + i, bursts, 4.0 - i)
        p = str(tmp_path / f'rec{i}.wav')
        with wave.open(p, 'wb') as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes((np.clip(sig, -1, 1) * 32767).astype('<i2').tobytes())
        paths.append(p)
    kw_file = str(tmp_path / 'kw.txt')
    with open(kw_file, 'w') as f:
        f.write('the\n\n  a cat  \noo\n')
    ckpt = str(tmp_path / 'model.ckpt')
    torch.save({'state_dict': model.state_dict()}, ckpt)
    out = str(tmp_path / 'hits.jsonl')
    records = S.main([f'model_path={ckpt}', 'audio=' + ','.join(paths), f'keywords={kw_file}', 'model.mid_layers=1', 'batch_size=1',
                      'threshold=-40', 'max_hits=3', f'output={out}'])
    lines = [json.loads(l) for l in open(out)]
    assert [l['path'] for l in lines] == paths and lines == json.loads(json.dumps(records))
    want = model.find_keywords([read_audio(p)[0] for p in paths], PHRASES, batch_size=1, **LOOSE)
    assert [l['hits'] for l in lines] == json.loads(json.dumps(want)) and all(l['hits'] for l in lines)
    for bad in (['max_hits=0'], ['threshold=x'], []):
        args = [f'model_path={ckpt}', f'audio={paths[0]}'] + ([f'keywords={kw_file}'] if bad else []) + bad
        with pytest.raises(SystemExit):
            S.main(args)


def test_find_keywords_under_asg_is_refused():
    from asg_replay_worker import build_model
    asg = build_model(seed=6).cuda().eval()
    with pytest.raises(NotImplementedError):
        asg.find_keywords([_speechlike(4, ((0.4, 1.2),), 2.0)], ['the'])
