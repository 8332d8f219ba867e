"""LJSpeech-format data path: the on-disk input of real training.

* ``LJSpeech(root)``: ``root/metadata.csv`` (``id|raw text|normalised text`` per line,
  pipe-separated, no header, as LJSpeech-1.1 ships it) and ``root/wavs/<id>.wav``
  (22.05 kHz mono PCM);
* ``text_to_ids``: a character front end -- lower-casing, the English abbreviation
  expansions of the Tacotron2 ``english_cleaners``, whitespace collapse, unknown
  characters dropped, an end-of-sentence id appended -- onto a 50-symbol table that
  fits the model's 80-id embedding (id 0 = pad).  Grapheme-to-phoneme conversion is
  out of scope; characters are what Tacotron2 trains on by default;
* ``bucket_batches``: length-bucketed, shuffled batches (similar lengths together, so
  padding -- and the masked compute it costs -- stays small);
* ``collate``: padded id / length tensors and log-mel targets [B, T, 80] computed on the
  GPU by ``tt2.audio.MelExtractor`` (one batched STFT per batch);
* ``extract_durations``: per-utterance phoneme durations from a trained model's alignment
  (``TransformerTTS.durations``), written as ``<id>.npy`` plus a ``durations.json`` manifest:
  the training targets of a non-autoregressive student.
* ``read_wav`` / ``LJSpeech(root, sr=...)`` / ``collate(..., resampler=)`` / ``resample_corpus``:
  corpora at other rates (LibriTTS 24 kHz, VCTK 48 kHz).  ``load_wav`` still refuses a file that is
  not at the rate it is asked for; ``resample_corpus`` (``tools/resample_corpus.py``) rewrites a
  corpus at 22.05 kHz through ``tt2.audio.Resampler``, and ``collate`` can run the same resampler on
  the fly.  Everything downstream (mels, pitch, durations, MCD) stays at 22.05 kHz.
* ``trim_corpus`` (``tools/trim_corpus.py``): the corpus with leading and trailing silence removed by
  ``tt2.audio.SilenceTrimmer`` (which can resample in the same pass), with a ``trim.json`` manifest;
  a SilenceTrimmer also fits ``collate(..., resampler=)`` as it is.
* ``normalize_corpus`` (``tools/normalize_corpus.py``): the corpus brought to one integrated loudness
  (ITU-R BS.1770) under a sample-peak ceiling by ``tt2.audio.LoudnessNormalizer`` (which can resample
  and trim in the same pass), with a ``loudness.json`` manifest; it fits ``collate(..., resampler=)``
  as well.
"""
from __future__ import annotations

import csv
import json
import os
import random
import re

import numpy as np
import torch

PAD, EOS = "_", "~"
_PUNCT = "!'(),.:;?-\""
SYMBOLS = [PAD, EOS, " "] + list(_PUNCT) + [chr(c) for c in range(ord("a"), ord("z") + 1)] + \
          [str(d) for d in range(10)]
SYMBOL_ID = {s: i for i, s in enumerate(SYMBOLS)}

_ABBREV = [(re.compile(r"\b%s\." % k, re.IGNORECASE), v) for k, v in [
    ("mrs", "misess"), ("mr", "mister"), ("dr", "doctor"), ("st", "saint"), ("co", "company"), ("jr", "junior"),
    ("maj", "major"), ("gen", "general"), ("drs", "doctors"), ("rev", "reverend"), ("lt", "lieutenant"),
    ("hon", "honorable"), ("sgt", "sergeant"), ("capt", "captain"), ("esq", "esquire"), ("ltd", "limited"),
    ("col", "colonel"), ("ft", "fort")]]
_WS = re.compile(r"\s+")


def clean_text(text: str) -> str:
    text = text.lower()
    for pat, rep in _ABBREV:
        text = pat.sub(rep, text)
    return _WS.sub(" ", text).strip()


def text_to_ids(text: str, eos: bool = True) -> list[int]:
    ids = [SYMBOL_ID[c] for c in clean_text(text) if c in SYMBOL_ID and c not in (PAD, EOS)]
    return ids + [SYMBOL_ID[EOS]] if eos else ids


def ids_to_text(ids) -> str:
    return "".join(SYMBOLS[i] for i in ids if 0 < i < len(SYMBOLS) and SYMBOLS[i] != EOS)


def read_wav(path: str) -> tuple[np.ndarray, int]:
    """(mono float32 in [-1, 1], rate) of a PCM16 / PCM32 / float WAV, at the file's own rate:
    load_wav's conversions, unchanged.  (Channels are averaged before the integer scaling is
    chosen, so a multi-channel PCM file comes out unscaled, as it always did from load_wav.)"""
    from scipy.io import wavfile
    rate, x = wavfile.read(path)
    if x.ndim > 1:
        x = x.mean(axis=1)
    if x.dtype == np.int16:
        return (x / 32768.0).astype(np.float32), int(rate)
    if x.dtype == np.int32:
        return (x / 2147483648.0).astype(np.float32), int(rate)
    return x.astype(np.float32), int(rate)


def load_wav(path: str, sr: int = 22050) -> np.ndarray:
    """Mono float32 in [-1, 1] (PCM16 / PCM32 / float WAV); no resampling."""
    x, rate = read_wav(path)
    if rate != sr:
        raise ValueError(f"{path}: {rate} Hz, expected {sr} (resample offline: tools/resample_corpus.py)")
    return x


class LJSpeech:
    def __init__(self, root: str, use_normalized: bool = True, sr: int = 22050):
        self.root = root
        self.sr = int(sr)   # the rate of the corpus' files: wav() refuses any other
        self.items = []   # (id, text)
        with open(os.path.join(root, "metadata.csv"), encoding="utf-8", newline="") as f:
            for row in csv.reader(f, delimiter="|", quoting=csv.QUOTE_NONE):
                if not row:
                    continue
                uid, raw = row[0], row[1]
                norm = row[2] if len(row) > 2 and row[2] else raw
                self.items.append((uid, norm if use_normalized else raw))

    def __len__(self):
        return len(self.items)

    def wav(self, i: int) -> np.ndarray:
        return load_wav(os.path.join(self.root, "wavs", self.items[i][0] + ".wav"), self.sr)

    def ids(self, i: int) -> list[int]:
        return text_to_ids(self.items[i][1])


def bucket_batches(lengths, batch_size: int, bucket_mult: int = 8, seed: int = 0, drop_last: bool = False):
    """Shuffle, cut into chunks of batch_size * bucket_mult, sort each chunk by length,
    split into batches, shuffle the batches: every index appears exactly once."""
    rng = random.Random(seed)
    idx = list(range(len(lengths)))
    rng.shuffle(idx)
    chunk = batch_size * bucket_mult
    batches = []
    for c in range(0, len(idx), chunk):
        part = sorted(idx[c:c + chunk], key=lambda i: lengths[i])
        for b in range(0, len(part), batch_size):
            bb = part[b:b + batch_size]
            if len(bb) == batch_size or not drop_last:
                batches.append(bb)
    rng.shuffle(batches)
    return batches


def pad_batch(wavs):
    """(audio [B, L] f32, lens [B] int32) on the host: the waveforms (1-D float32 arrays) as rows,
    zero-padded to the longest."""
    audio = torch.zeros(len(wavs), max(len(w) for w in wavs), dtype=torch.float32)
    for b, w in enumerate(wavs):
        audio[b, :len(w)] = torch.from_numpy(w)
    return audio, torch.tensor([len(w) for w in wavs], dtype=torch.int32)


def collate(ds: LJSpeech, indices, extractor, device="cuda", resampler=None):
    """(text [B, Tx] i64, text_len [B], mel [B, T, 80] f32, mel_len [B]) for one batch;
    the log-mels come from one batched GPU STFT (tt2.audio.MelExtractor).  With a resampler (a
    tt2.audio.Resampler whose sr_in is the corpus' rate ds.sr) the uploaded batch goes through it
    first and the extractor sees its output and output lengths."""
    if resampler is not None and int(resampler.sr_in) != int(getattr(ds, "sr", 22050)):
        raise ValueError(f"collate: the resampler reads {resampler.sr_in} Hz, the corpus is at "
                         f"{getattr(ds, 'sr', 22050)} Hz")
    ids = [ds.ids(i) for i in indices]
    wavs = [ds.wav(i) for i in indices]
    B = len(indices)
    tx = max(len(s) for s in ids)
    text = torch.zeros(B, tx, dtype=torch.long)
    for b, s in enumerate(ids):
        text[b, :len(s)] = torch.tensor(s)
    text_len = torch.tensor([len(s) for s in ids])
    audio, lens = (t.to(device) for t in pad_batch(wavs))
    if resampler is not None:
        audio, lens = resampler(audio, lens)
    mel, frames = extractor(audio, lens)
    return text.to(device), text_len.to(device), mel, frames.to(torch.long)


def extract_durations(model, batches, out_dir: str, head="best", method="argmax"):
    """Phoneme durations of every utterance in `batches`, an iterable (re-iterable for
    head="dataset") of (ids, text, text_len, mel, mel_len), through
    model.durations(text, text_len, mel, mel_len, head=...).  head:
      "best"     each utterance's own best (layer, head);
      "dataset"  two passes: the first accumulates the frame-weighted focus rate of every
                 (layer, head) over all utterances (model.alignment_stats() after each
                 durations() forward), the second uses the single head with the highest one;
      (l, h)     that head.
    Writes out_dir/<id>.npy (int32 [text_len]) per utterance and out_dir/durations.json:
    {"head": ..., "utterances": {id: {"layer", "head", "focus", "frames", "phonemes"}}}.
    Returns the manifest.  The model needs only durations() (and alignment_stats() for
    "dataset"), so a stub drives it in tests.

    method="argmax" (the default) counts each frame's strongest phoneme (model.durations());
    method="monotonic" takes the durations of the monotonic alignment search instead
    (model.monotonic_durations(): every phoneme gets a frame when frames >= phonemes, and the
    frames never go back).  The manifest then carries "method", per utterance the path's "logp"
    and "min_duration" (0 marks an utterance with fewer frames than phonemes).  The head="dataset"
    pass that picks the head is the same for both.

    Batch shapes: the engine keeps one arena of activations per distinct (B, Tx, Ty) it has run,
    for good (about 110 KB per decoder row in bf16: about 1.1 GB at B = 16 and 650 frames), and
    ragged batches as bucket_batches + collate make them nearly all differ: a corpus would hold
    hundreds of arenas.  So every call here is durations(..., transient=True): an arena that the
    call itself created is dropped again afterwards (it stays alive as the model's last forward
    until the next one, so at most two are held), while the arena of a shape the model already
    ran (its training shape, a captured step's) is left alone.  The batches are not padded or
    otherwise changed: padding an utterance further changes what the encoder's convolutions see
    at its end, and with it the alignment."""
    if method not in ("argmax", "monotonic"):
        raise ValueError(f'extract_durations: method must be "argmax" or "monotonic", got {method!r}')
    mono = method == "monotonic"
    os.makedirs(out_dir, exist_ok=True)
    use = head
    dataset_focus = None
    if isinstance(head, str) and head == "dataset":
        if iter(batches) is batches:
            raise ValueError('extract_durations: head="dataset" reads the batches twice; pass a list, not an iterator')
        num = None
        frames = 0.0
        layers = None
        for _, text, text_len, mel, mel_len in batches:
            model.durations(text, text_len, mel, mel_len, head="best", transient=True)
            st = model.alignment_stats()
            w = torch.as_tensor(mel_len).to(st.focus.device, torch.float64).clamp(max=mel.shape[1])
            part = (st.focus.to(torch.float64) * w[None, :, None]).sum(1)   # [L, H], frame-weighted
            num = part if num is None else num + part
            frames += float(w.sum())
            layers = tuple(st.layers)
        if num is None:
            raise ValueError("extract_durations: no batches")
        flat = int(torch.argmax(num.reshape(-1)))   # the lowest flat index on ties
        use = (int(layers[flat // num.shape[1]]), flat % num.shape[1])
        dataset_focus = float(num.reshape(-1)[flat]) / max(frames, 1.0)
    elif not (isinstance(head, str) and head == "best"):
        use = (int(head[0]), int(head[1]))
    manifest = {"head": head if isinstance(head, str) else list(use), "utterances": {}}
    if dataset_focus is not None:
        manifest["dataset_head"] = list(use)
        manifest["dataset_focus"] = dataset_focus
    if mono:
        manifest["method"] = method
    for ids, text, text_len, mel, mel_len in batches:
        run = model.monotonic_durations if mono else model.durations
        r = run(text, text_len, mel, mel_len, head=use, transient=True)
        lp = r.logp.cpu().numpy() if mono else None
        dur, hd, fc = r.durations.cpu().numpy(), r.head.cpu().numpy(), r.focus.cpu().numpy()
        tl = [int(x) for x in torch.as_tensor(text_len).cpu()]
        ml = [int(x) for x in torch.as_tensor(mel_len).cpu()]
        for b, uid in enumerate(ids):
            d = np.ascontiguousarray(dur[b, :tl[b]], dtype=np.int32)
            np.save(os.path.join(out_dir, f"{uid}.npy"), d)
            manifest["utterances"][str(uid)] = {"layer": int(hd[b, 0]), "head": int(hd[b, 1]), "focus": float(fc[b]),
                                                "frames": min(ml[b], mel.shape[1]), "phonemes": tl[b]}
            if mono:
                manifest["utterances"][str(uid)].update(logp=float(lp[b]), min_duration=int(d.min()) if d.size else 0)
    with open(os.path.join(out_dir, "durations.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    return manifest


def extract_pitch(batches, out_dir: str, extractor, durations_dir: str | None = None):
    """Frame-level pitch and energy of every utterance in `batches`, an iterable of
    (ids, audio [B, L], lens [B] samples), through extractor(audio, lens) -> a tt2.audio.Pitch
    (f0, voiced, aperiodicity, energy, frames): a tt2.audio.PitchExtractor, or a stub in tests.
    Writes per utterance out_dir/<id>.f0.npy and <id>.energy.npy (f32 [frames]; f0 is 0 where
    unvoiced).  Where durations_dir holds <id>.npy (extract_durations' output), also
    <id>.f0_ph.npy and <id>.energy_ph.npy (f32 [phonemes]): tt2.audio.phoneme_average over each
    phoneme's frames, the pitch over its voiced frames only (0 for a phoneme without one).  An
    utterance whose durations do not sum to its frame count is refused with a ValueError that
    names it.  Writes out_dir/pitch.json: {"extractor": its params(), "utterances": {id:
    {"frames", "voiced"}} with voiced the share of voiced frames, "log_f0": {"mean", "std",
    "frames"} over all voiced frames (natural log), "energy": {"mean", "std", "frames"} over
    all frames}; the standard deviations are the population ones.  Returns the manifest."""
    from .audio import phoneme_average
    os.makedirs(out_dir, exist_ok=True)
    params = extractor.params() if hasattr(extractor, "params") else {}
    manifest = {"extractor": params, "utterances": {}}
    acc = {"log_f0": [0, 0.0, 0.0], "energy": [0, 0.0, 0.0]}   # count, sum, sum of squares (float64 on the host)

    def add(key, x):
        x = x.astype(np.float64)
        acc[key][0] += x.size
        acc[key][1] += float(x.sum())
        acc[key][2] += float((x * x).sum())

    for ids, audio, lens in batches:
        p = extractor(audio, lens)
        f0, energy = p.f0.detach().float().cpu(), p.energy.detach().float().cpu()
        voiced = p.voiced.detach().cpu()
        frames = [int(n) for n in torch.as_tensor(p.frames).cpu()]
        for b, uid in enumerate(ids):
            n = min(frames[b], f0.shape[1])
            f, e, v = f0[b, :n].numpy(), energy[b, :n].numpy(), voiced[b, :n].numpy().astype(bool)
            np.save(os.path.join(out_dir, f"{uid}.f0.npy"), np.ascontiguousarray(f, dtype=np.float32))
            np.save(os.path.join(out_dir, f"{uid}.energy.npy"), np.ascontiguousarray(e, dtype=np.float32))
            manifest["utterances"][str(uid)] = {"frames": n, "voiced": float(v.mean()) if n else 0.0}
            add("log_f0", np.log(f[v].astype(np.float64)))
            add("energy", e)
            dpath = os.path.join(durations_dir, f"{uid}.npy") if durations_dir else None
            if dpath and os.path.exists(dpath):
                d = np.load(dpath)
                if int(d.sum()) != n:
                    raise ValueError(f"extract_pitch: durations of {uid} sum to {int(d.sum())} frames, "
                                     f"its audio has {n}")
                dt_ = torch.from_numpy(d.astype(np.int64))[None]
                f_ph = phoneme_average(f0[b:b + 1, :n], dt_, voiced[b:b + 1, :n])[0].numpy()
                e_ph = phoneme_average(energy[b:b + 1, :n], dt_)[0].numpy()
                np.save(os.path.join(out_dir, f"{uid}.f0_ph.npy"), np.ascontiguousarray(f_ph, dtype=np.float32))
                np.save(os.path.join(out_dir, f"{uid}.energy_ph.npy"), np.ascontiguousarray(e_ph, dtype=np.float32))
    for key, (cnt, s, s2) in acc.items():
        mean = s / cnt if cnt else 0.0
        manifest[key] = {"mean": mean, "std": max(s2 / cnt - mean * mean, 0.0) ** 0.5 if cnt else 0.0, "frames": cnt}
    with open(os.path.join(out_dir, "pitch.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    return manifest


def _numbers(t, kind=int):
    return [kind(v) for v in torch.as_tensor(t).cpu()]


def _corpus_pass(who, ds, out_root, stage, batch_size, run, entry, key, manifest_name, skip_empty=True, totals=None):
    """One pass of a waveform stage over the corpus `ds` into a corpus of the same layout under
    out_root; what resample_corpus, trim_corpus and normalize_corpus share.  Per batch of batch_size
    utterances in corpus order: run(audio [B, L], lens [B]) -> (audio_out, out_lens, extras), extras a
    tuple of per-utterance lists; per utterance: out_root/wavs/<id>.wav (PCM16 mono at stage.sr_out:
    rint(x * 32768) clipped to [-32768, 32767]) and entry(uid, samples_in, samples_out, clipped,
    *its extras) -> its manifest entry.  With skip_empty an utterance of no samples is not written,
    is listed under "empty", and its line is left out of the copied metadata.csv.  totals() -> the
    corpus-level keys.  Writes out_root/<manifest_name>: {key: stage.params(), "utterances": ...}
    and returns it."""
    import shutil
    from scipy.io import wavfile
    sr = getattr(ds, "sr", 22050)
    if int(stage.sr_in) != int(sr):
        raise ValueError(f"{who}: the stage reads {stage.sr_in} Hz, the corpus is at {sr} Hz")
    if batch_size < 1:
        raise ValueError(f"{who}: batch_size must be at least 1")
    if os.path.abspath(out_root) == os.path.abspath(ds.root):
        raise ValueError(f"{who}: out_root is the corpus itself")
    os.makedirs(os.path.join(out_root, "wavs"), exist_ok=True)
    dev = getattr(stage, "dev", "cpu")
    manifest = {key: stage.params() if hasattr(stage, "params") else {}, "utterances": {}}
    empty = []
    if skip_empty:
        manifest["empty"] = empty
    for s in range(0, len(ds), batch_size):
        idx = list(range(s, min(s + batch_size, len(ds))))
        wavs = [ds.wav(i) for i in idx]
        audio, lens = pad_batch(wavs)
        y, out_lens, extras = run(audio.to(dev), lens.to(dev))
        y = torch.as_tensor(y).detach().float().cpu().numpy()
        out_lens = _numbers(out_lens)
        for b, i in enumerate(idx):
            uid = str(ds.items[i][0])
            q = np.rint(y[b, :out_lens[b]].astype(np.float64) * 32768.0)
            clipped = int(((q < -32768) | (q > 32767)).sum())
            manifest["utterances"][uid] = entry(uid, len(wavs[b]), out_lens[b], clipped, *(e[b] for e in extras))
            if skip_empty and out_lens[b] == 0:
                empty.append(uid)
                continue
            wavfile.write(os.path.join(out_root, "wavs", uid + ".wav"), int(stage.sr_out),
                          np.clip(q, -32768, 32767).astype(np.int16))
    if totals is not None:
        manifest.update(totals())
    src, dst = os.path.join(ds.root, "metadata.csv"), os.path.join(out_root, "metadata.csv")
    if not empty:
        shutil.copyfile(src, dst)
    else:
        gone = set(empty)
        with open(src, encoding="utf-8", newline="") as f, open(dst, "w", encoding="utf-8", newline="") as g:
            for line in f:
                if line.split("|", 1)[0].rstrip("\r\n") not in gone:
                    g.write(line)
    with open(os.path.join(out_root, manifest_name), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    return manifest


def resample_corpus(ds: LJSpeech, out_root: str, resampler, batch_size: int = 16):
    """The corpus `ds` at the resampler's output rate, as a corpus of the same layout under
    out_root: out_root/wavs/<id>.wav (PCM16 mono at sr_out: rint(x * 32768) clipped to
    [-32768, 32767]), a copy of metadata.csv, and out_root/resample.json: {"resampler": its
    params(), "utterances": {id: {"samples_in", "samples_out", "clipped"}}} with `clipped` the
    number of samples the PCM16 range cut.  `resampler` is a tt2.audio.Resampler whose sr_in is
    ds.sr, or any callable (audio [B, L], lens [B]) -> (audio_out, out_lens) with sr_in, sr_out and
    params(): one call per batch of batch_size utterances in corpus order.  Returns the manifest."""
    def entry(uid, samples_in, samples_out, clipped):
        return {"samples_in": samples_in, "samples_out": samples_out, "clipped": clipped}

    return _corpus_pass("resample_corpus", ds, out_root, resampler, batch_size,
                        lambda audio, lens: (*resampler(audio, lens), ()), entry, "resampler", "resample.json",
                        skip_empty=False)


def trim_corpus(ds: LJSpeech, out_root: str, trimmer, batch_size: int = 16):
    """The corpus `ds` with leading and trailing silence removed, as a corpus of the same layout
    under out_root: out_root/wavs/<id>.wav (PCM16 mono at the trimmer's sr_out: rint(x * 32768)
    clipped to [-32768, 32767]), a copy of metadata.csv, and out_root/trim.json: {"trimmer": its
    params(), "utterances": {id: {"samples_in", "start", "samples_out", "clipped"}},
    "removed_seconds": samples_in / sr_in - samples_out / sr_out summed over the corpus,
    "empty": [ids]}.  `start` and `samples_out` count samples at sr_out (after the trimmer's
    resampler, when it has one).  An utterance trimmed to nothing is not written: it is listed under
    "empty" and its line is left out of the copied metadata.csv, so that nothing downstream meets a
    zero-length file.  `trimmer` is a tt2.audio.SilenceTrimmer whose sr_in is ds.sr, or any object
    with sr_in, sr_out, params() and trim(audio [B, L], lens [B]) -> (audio, lens, start, energy):
    one call per batch of batch_size utterances in corpus order.  Returns the manifest."""
    sr_in, sr_out, removed = int(trimmer.sr_in), int(trimmer.sr_out), [0.0]

    def run(audio, lens):
        y, out_lens, start = trimmer.trim(audio, lens)[:3]
        return y, out_lens, (_numbers(start),)

    def entry(uid, samples_in, samples_out, clipped, start):
        removed[0] += samples_in / sr_in - samples_out / sr_out
        return {"samples_in": samples_in, "start": start, "samples_out": samples_out, "clipped": clipped}

    return _corpus_pass("trim_corpus", ds, out_root, trimmer, batch_size, run, entry, "trimmer", "trim.json",
                        totals=lambda: {"removed_seconds": removed[0]})


def normalize_corpus(ds: LJSpeech, out_root: str, normalizer, batch_size: int = 16):
    """The corpus `ds` brought to one loudness, as a corpus of the same layout under out_root:
    out_root/wavs/<id>.wav (PCM16 mono at the normaliser's sr_out: rint(x * 32768) clipped to
    [-32768, 32767]), a copy of metadata.csv, and out_root/loudness.json: {"normalizer": its params(),
    "utterances": {id: {"samples", "loudness_in" (LKFS; null: unmeasured), "gain_db", "peak_in",
    "limited", "clipped"}}, "unmeasured": [ids], "empty": [ids], "stats": {"measured",
    "mean_loudness_in", "min_loudness_in", "max_loudness_in", "limited"}}.  An unmeasured utterance (no
    400 ms block above the gates: too short, or silence) is written at gain 1 and listed under
    "unmeasured"; the statistics run over the measured ones (null where there is none).  `samples`
    counts samples at sr_out (after the normaliser's resampler or trimmer, when it has one); an
    utterance that a trimmer in front left nothing of is listed under "empty" as well, not written,
    and its line is left out of the copied metadata.csv, as trim_corpus does.  `normalizer` is a
    tt2.audio.LoudnessNormalizer whose sr_in is ds.sr, or any object with sr_in, sr_out, params() and
    normalize(audio [B, L], lens [B]) -> (audio, lens, loud, gain, peak, limited): one call per batch
    of batch_size utterances in corpus order.  Returns the manifest."""
    import math
    measured, n_limited, unmeasured = [], [0], []

    def run(audio, lens):
        y, out_lens, loud, gain, peak, limited = normalizer.normalize(audio, lens)[:6]
        return y, out_lens, (_numbers(loud, float), _numbers(gain, float), _numbers(peak, float), _numbers(limited))

    def entry(uid, samples_in, samples_out, clipped, loud, gain, peak, limited):
        ok = math.isfinite(loud)
        if ok:
            measured.append(loud)
            n_limited[0] += limited
        else:
            unmeasured.append(uid)
        return {"samples": samples_out, "loudness_in": loud if ok else None,
                "gain_db": 20.0 * math.log10(gain) if gain > 0 else None,
                "peak_in": peak, "limited": bool(limited), "clipped": clipped}

    def totals():
        return {"unmeasured": unmeasured,
                "stats": {"measured": len(measured), "limited": n_limited[0],
                          "mean_loudness_in": sum(measured) / len(measured) if measured else None,
                          "min_loudness_in": min(measured) if measured else None,
                          "max_loudness_in": max(measured) if measured else None}}

    return _corpus_pass("normalize_corpus", ds, out_root, normalizer, batch_size, run, entry, "normalizer",
                        "loudness.json", totals=totals)
