"""Evaluation of a finished model over a data loader: the loop behind ``Trainer.test``, the ``test`` command line and
``ConvCTCASR.transcribe``.  Forward = ``model.infer`` (the fused inference engine), decoding = any decoder of this package,
metrics = corpus level: errors summed over the set divided by reference lengths summed over the set, with
``Decoder.cer_ratio`` / ``Decoder.wer_ratio`` arithmetic."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple


def corpus_metrics(decoder, pairs: Sequence[Tuple[str, str]]) -> Dict[str, float]:
    """(reference, hypothesis) pairs -> test_cer / test_wer / test_len_ratio over the whole set.  CER: character edit
    distances (spaces removed) summed / reference characters summed; WER: word edit distances summed / reference words
    summed; length ratio: hypothesis characters / reference characters.  An empty denominator gives 0.0 for an error-free
    set and inf otherwise."""
    c_err = c_ref = w_err = w_ref = h_len = r_len = 0
    for ref, hyp in pairs:
        e, d = decoder.cer_ratio(ref, hyp)
        c_err, c_ref = c_err + e, c_ref + d
        e, d = decoder.wer_ratio(ref, hyp)
        w_err, w_ref = w_err + e, w_ref + d
        h_len, r_len = h_len + len(hyp), r_len + len(ref)

    def ratio(a, b):
        return a / b if b else (0.0 if not a else float('inf'))

    return {'test_cer': ratio(c_err, c_ref), 'test_wer': ratio(w_err, w_ref), 'test_len_ratio': ratio(h_len, r_len)}


def frame_seconds(model) -> float:
    """seconds per output frame: the feature hop times the network's stride product"""
    return float(model.audio_conf['window_stride']) * float(model.scaling_factor)


def decode_batch(model, decoder, out, out_lens, word_times: bool = False):
    """posteriors of one batch -> (hypotheses, word timings or Nones).  Word timings: forced alignment of each decoded string
    to the utterance's own frames (``Decoder.align``), then ``get_time_per_word(end_offsets=)``: (word, start s, end s)."""
    if getattr(getattr(model, 'criterion', None), 'is_asg', False):
        # a model trained with ASG has no blank: the CTC decoders and the CTC forced alignment do not apply to its output
        from .asg import ASGDecoder
        if not isinstance(decoder, ASGDecoder):
            raise NotImplementedError(f'{type(decoder).__name__} on a model with criterion asg: the CTC decoders and the CTC beam '
                                      'search know no transitions; use an asg.ASGDecoder (the model\'s own Viterbi decoder, or '
                                      'asg_beam.ASGBeamSearchDecoder / ASGBeamSearchLMDecoder)')
        if word_times:
            raise NotImplementedError('word_times under criterion asg is not wired in here: forced alignment under ASG is '
                                      'ASGDecoder.align (asg_beam.asg_forced_align)')
    hyps = decoder.decode(out, out_lens)
    hyps = [h[0] if isinstance(h, (list, tuple)) else h for h in hyps]
    if not word_times:
        return hyps, [None] * len(hyps)
    from .beam_search import get_time_per_word
    ratio = frame_seconds(model)
    log_probs = bool(getattr(model, 'infer_log_probs', True))
    words = []
    for n, hyp in enumerate(hyps):
        if not hyp.strip():
            words.append([])
            continue
        size = None if out_lens is None else out_lens[n: n + 1]
        offs, ends = decoder.align(out[n: n + 1], [hyp], sizes=size, log_probs=log_probs)
        words.append([(w, float(s), float(e)) for w, s, e in
                      get_time_per_word(hyp, offs[0][0].tolist(), ratio, end_offsets=ends[0][0].tolist())])
    return hyps, words


def add_error_counts(records: List[dict], metrics: Dict[str, float]) -> None:
    """what the errors are made of: every (text, hypothesis) pair of the set scored by ONE mbr.edit_distance_gpu(...,
    counts=True) per unit -> ``word_sub`` / ``word_del`` / ``word_ins`` and the ``char`` trio in each record (they sum to its
    word_errors / char_errors), ``test_word_sub`` ... ``test_char_ins`` in the metrics: each count summed over the set divided
    by the summed reference length (0.0 / inf on an empty denominator, as corpus_metrics).  A transcript or hypothesis of more
    than 4095 words / characters is edit_distance_gpu's ValueError."""
    from .mbr import edit_distance_gpu
    refs, hyps = [r['text'] for r in records], [r['hypothesis'] for r in records]
    for unit in ('word', 'char'):
        _, counts = edit_distance_gpu(refs, hyps, unit=unit, counts=True)
        ref_len = sum(r[unit + '_ref'] for r in records)
        for col, kind in enumerate(('sub', 'del', 'ins')):
            for r, row in zip(records, counts):
                r['%s_%s' % (unit, kind)] = int(row[col])
            total = int(counts[:, col].sum()) if len(records) else 0
            metrics['test_%s_%s' % (unit, kind)] = total / ref_len if ref_len else (0.0 if not total else float('inf'))


def evaluate(model, dataloader, decoder=None, word_times: bool = False,
             error_counts: bool = False) -> Tuple[Dict[str, float], List[dict]]:
    """``model.infer`` over every batch of ``dataloader`` (the 6-tuples of data_loader._collator) -> (metrics, records):
    metrics = test_loss (batch-size-weighted mean of the batch losses, as the validation epoch mean is formed), test_cer,
    test_wer, test_len_ratio (corpus_metrics); one record per utterance with path, text, hypothesis, char_errors, char_ref,
    word_errors, word_ref (and words with ``word_times``).  ``error_counts``: add_error_counts' keys on both."""
    import torch
    decoder = decoder or model.ctc_decoder
    was_training = model.training
    model.eval()
    records: List[dict] = []
    loss_sum, n_sum = 0.0, 0
    try:
        with torch.no_grad():
            for batch in dataloader:
                spect, spect_lens, targets, target_lens, paths, texts = batch
                if hasattr(model, 'metric_texts'):
                    texts = model.metric_texts(texts)          # model.wildcard: scored without the mark (upper bounds)
                x = model._device_batch(spect)
                out, out_lens = model.infer(x, spect_lens)
                if x.is_cuda and all(torch.is_tensor(t) for t in (out_lens, targets, target_lens)):
                    tg_d, ol_d, tl_d = model._device_ints(x.device, targets, out_lens, target_lens)
                else:
                    tg_d, ol_d, tl_d = targets, out_lens, target_lens
                loss = model.criterion(out.transpose(0, 1), tg_d, ol_d, tl_d)
                hyps, words = decode_batch(model, decoder, out, out_lens, word_times)
                loss_sum += float(loss) * len(texts)
                n_sum += len(texts)
                for path, text, hyp, w in zip(paths, texts, hyps, words):
                    ce, cr = decoder.cer_ratio(text, hyp)
                    we, wr = decoder.wer_ratio(text, hyp)
                    rec = {'path': path, 'text': text, 'hypothesis': hyp, 'char_errors': int(ce), 'char_ref': int(cr),
                           'word_errors': int(we), 'word_ref': int(wr)}
                    if word_times:
                        rec['words'] = [{'word': a, 'start': s, 'end': e} for a, s, e in w]
                    records.append(rec)
    finally:
        if was_training:
            model.train()
    metrics = {'test_loss': loss_sum / n_sum if n_sum else float('nan')}
    metrics.update(corpus_metrics(decoder, [(r['text'], r['hypothesis']) for r in records]))
    if error_counts:
        add_error_counts(records, metrics)
    return metrics, records
