"""mel_batch.py: the ragged batch of whole-file log-mels and everything that hands one to a `wm_*` mel entry point.

transcribe.py's layers all read the same batch or one derived from it.  `MelBatch` holds it -- the mels as contiguous fp16
[n_mels, frames] tensors on the GPU, their content frames -- with the one validation and the device table of pointers, row lengths
and content frames, checked and uploaded at first use and then kept.  Every wrapper below takes `(mels, content_frames, ...)` as
lists, or a `MelBatch` in place of `mels` (`content_frames` is then the batch's own): a caller that holds a batch neither validates
nor uploads it again.

  mel_windows   wm_mel_windows   (csrc/windows.hip)    a round's windows, each at its own seek; its table changes every round
  section_cuts  wm_section_cuts  (csrc/sections.hip)   where every file is quietest            } counts, then payload: one copy
  speech_spans  wm_speech_spans  (csrc/speech.hip)     what an energy rule takes for speech    } back for all files
  packed_mels   wm_mel_gather    (csrc/speech.hip)     the spans' columns as shorter files
  section_mels  (torch slices)                         the sections as files of their own
  channel_top   wm_channel_top   (csrc/channels.hip)   the loudest channel of every frame, and the gate
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

import channels as channels_mod
import native
import sections as sections_mod
import speech as speech_mod
from channels import ChannelOptions
from sections import SectionOptions
from speech import SpeechOptions


def _is_mel(m: torch.Tensor, n_mels: int) -> bool:
    return m.is_cuda and m.dtype == torch.float16 and m.dim() == 2 and m.shape[0] == n_mels and m.is_contiguous()


_NOT_A_MEL = "a mel must be a contiguous fp16 [n_mels, frames] tensor on the GPU"


class MelBatch(list):
    """A ragged batch of whole-file mels: the list of the mels, which also knows their `content_frames` (and their sum, `total`),
    `n_mels`, the `device` and, from the first use on, the device `table` (int64 [3, n]: pointers, row lengths, content frames).
    `what` heads the errors.  The mels are taken as they are; they are checked when the table is built."""

    def __init__(self, mels: Sequence[torch.Tensor], content_frames: Sequence[int], what: str = "transcribe"):
        if len(content_frames) != len(mels):
            raise ValueError(f"{what}: {len(content_frames)} content_frames for {len(mels)} mels")
        super().__init__(mels)
        self.content_frames = [int(c) for c in content_frames]
        self.total = sum(self.content_frames)
        self.n_mels = int(self[0].shape[0]) if self else 0
        self.device = self[0].device if self else None
        self.what = what
        self.table: Optional[torch.Tensor] = None
        self._rows = None

    @classmethod
    def of(cls, mels, content_frames, what: str) -> "MelBatch":
        return mels if isinstance(mels, cls) else cls(mels, content_frames, what)

    def check_bins(self, n_mels: int) -> None:
        """Refuse a batch whose mels do not have the engine's `n_mels` bins (80 up to large-v2, 128 from large-v3 on)."""
        for f, m in enumerate(self):
            if m.dim() != 2 or int(m.shape[0]) != int(n_mels):
                raise ValueError(f"{self.what}: mel {f} has shape {tuple(m.shape)}, the engine takes mels of {int(n_mels)} bins")

    def rows(self):
        """(pointers, row lengths, content frames) as device addresses of int64 [n], int32 [n], int32 [n]: the three arrays every
        mel entry point reads.  The first call validates the batch and uploads the table; later ones return what is there."""
        if self.table is None:
            for m, c in zip(self, self.content_frames):
                assert _is_mel(m, self.n_mels), _NOT_A_MEL
                if not 0 <= c <= m.shape[1]:
                    raise ValueError(f"{self.what}: {c} frames of content in a mel of {m.shape[1]}")
            self.table = torch.tensor([[m.data_ptr() for m in self], [m.shape[1] for m in self], self.content_frames],
                                      dtype=torch.int64).to(self.device, non_blocking=False)
            self._rows = (self.table[0], self.table[1].to(torch.int32), self.table[2].to(torch.int32))
        return tuple(t.data_ptr() for t in self._rows)


def mel_windows(mels: Sequence[Optional[torch.Tensor]], seeks: Sequence[int], n_mels: int, n_window: int,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp16 [len(mels), n_mels, n_window]: row b is mels[b][:, seeks[b] : seeks[b] + n_window], zero behind the mel's end and
    all zero for a None entry (wm_mel_windows: one launch for the ragged batch, on the current stream)."""
    n = len(mels)
    assert n >= 1 and len(seeks) == n
    dev = next((m.device for m in mels if m is not None), out.device if out is not None else torch.device("cuda"))
    for m in mels:
        assert m is None or _is_mel(m, n_mels), _NOT_A_MEL
    table = torch.tensor([[0 if m is None else m.data_ptr() for m in mels],
                          [0 if m is None else m.shape[1] for m in mels],
                          [int(s) for s in seeks]], dtype=torch.int64).to(dev, non_blocking=False)
    frames, seek = table[1].to(torch.int32), table[2].to(torch.int32)
    if out is None:
        out = torch.empty((n, n_mels, n_window), dtype=torch.float16, device=dev)
    assert out.shape == (n, n_mels, n_window) and out.dtype == torch.float16 and out.is_contiguous()
    native.check(native.load_library().wm_mel_windows(table[0].data_ptr(), frames.data_ptr(), seek.data_ptr(), n, n_mels, n_window,
                                                      out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "wm_mel_windows")
    return out


def _counted(batch: MelBatch, what: str, ld: int, width: int, things: str, launch: Callable[[int, int], int]) -> List[List[int]]:
    """The read-back of an entry point that writes counts [n] and a payload [n][ld][width] of int32: one buffer, `launch(payload
    address, counts address)`, one copy back, and per file the width * count values it found."""
    n, entry = len(batch), "wm_" + what
    out = torch.empty(n * (1 + width * ld), dtype=torch.int32, device=batch.device)
    native.check(launch(out[n:].data_ptr(), out.data_ptr()), entry)
    host = out.cpu().tolist()
    found = host[:n]
    if any(k < 0 or k > ld for k in found):
        raise ValueError(f"{what}: {entry} found {found} {things}, room for {ld} per file")
    return [host[n + width * f * ld: n + width * (f * ld + found[f])] for f in range(n)]


def section_cuts(mels, content_frames: Optional[Sequence[int]], options: SectionOptions, window: int = 3000) -> List[List[int]]:
    """The cut frames of every file, ascending (sections.section_cuts_ref on the device: ONE wm_section_cuts launch for all files on
    the current stream and one copy of the cuts and their counts back).  mels[f]: contiguous fp16 [n_mels, >= content_frames[f]]
    on the GPU; `window`: the model's 2 * n_audio_ctx, which fixes the seconds per frame."""
    batch = MelBatch.of(mels, content_frames, "section_cuts")
    n = len(batch)
    if n == 0:
        return []
    lo, hi, h = options.frames(window, batch.n_mels)
    src, ld, content = batch.rows()
    lib, stream = native.load_library(), torch.cuda.current_stream(batch.device).cuda_stream
    ws_bytes = int(lib.wm_section_cuts_workspace_bytes(n, batch.total))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=batch.device)
    cuts_ld = max(1, max(batch.content_frames) // lo)
    return _counted(batch, "section_cuts", cuts_ld, 1, "cuts", lambda cuts, n_cuts: lib.wm_section_cuts(
        src, ld, content, n, batch.n_mels, lo, hi, h, cuts, cuts_ld, n_cuts, ws.data_ptr(), ws_bytes, batch.total, stream))


def speech_spans(mels, content_frames: Optional[Sequence[int]], options: SpeechOptions, window: int = 3000) -> List[List[tuple]]:
    """The speech spans [(a, b), ...] of every file in frames, ascending (speech.speech_spans_ref on the device: ONE wm_speech_spans
    launch for all files on the current stream and one copy of the spans and their counts back).  mels[f]: contiguous fp16
    [n_mels, >= content_frames[f]] on the GPU; `window`: the model's 2 * n_audio_ctx, which fixes the seconds per frame."""
    batch = MelBatch.of(mels, content_frames, "speech_spans")
    n = len(batch)
    if n == 0:
        return []
    src, ld, content = batch.rows()
    h, step, permille, min_silence, min_speech, pad = options.frames(window, batch.n_mels)
    lib, stream = native.load_library(), torch.cuda.current_stream(batch.device).cuda_stream
    ws_bytes = int(lib.wm_speech_spans_workspace_bytes(n, batch.total))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=batch.device)
    # rule (b) leaves gaps of at least min_silence frames between spans of at least one frame, and (c), (d) only take spans away
    spans_ld = max(1, (max(batch.content_frames) + min_silence) // (1 + min_silence))
    flat = _counted(batch, "speech_spans", spans_ld, 2, "spans", lambda spans, n_spans: lib.wm_speech_spans(
        src, ld, content, n, batch.n_mels, h, step, permille, min_silence, min_speech, pad, spans, spans_ld, n_spans, ws.data_ptr(),
        ws_bytes, batch.total, stream))
    return [list(zip(x[0::2], x[1::2])) for x in flat]


def packed_mels(mels, content_frames: Optional[Sequence[int]], spans: Sequence[Sequence[tuple]], window: int):
    """(packed mels, their content frames P): per file the columns of its spans in order, then `window` copies of its last column
    -- speech.packed_mel_ref's bit for bit, [n_mels, P + window] each -- from ONE wm_mel_gather launch for all files."""
    batch = MelBatch.of(mels, content_frames, "packed_mels")
    n, n_mels, dev = len(batch), batch.n_mels, batch.device
    if n == 0:
        return [], []
    if len(spans) != n:
        raise ValueError(f"packed_mels: {len(spans)} span lists for {n} mels")
    src, ld, _ = batch.rows()
    for m, c, sp in zip(batch, batch.content_frames, spans):
        if m.shape[1] < 1:
            raise ValueError("packed_mels: a mel without frames")
        speech_mod.check_spans(sp, c)
    packed = [sum(b - a for a, b in sp) for sp in spans]
    out = [torch.empty((n_mels, P + window), dtype=torch.float16, device=dev) for P in packed]
    spans_ld = max(1, max(len(sp) for sp in spans))
    flat = [[v for a, b in sp for v in (a, b)] + [0] * (2 * (spans_ld - len(sp))) for sp in spans]
    ints = torch.tensor([len(sp) for sp in spans] + [P + window for P in packed] + [v for row in flat for v in row],
                        dtype=torch.int32).to(dev, non_blocking=False)              # n_spans [n], dst_ld [n], spans [n][spans_ld][2]
    dst = torch.tensor([o.data_ptr() for o in out], dtype=torch.int64).to(dev, non_blocking=False)
    native.check(native.load_library().wm_mel_gather(src, ld, ints[2 * n:].data_ptr(), ints.data_ptr(), spans_ld, n, n_mels, window,
                                                     dst.data_ptr(), ints[n:].data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                 "wm_mel_gather")
    return out, packed


def section_mels(mels: Sequence[torch.Tensor], content_frames: Sequence[int], cuts: Sequence[Sequence[int]], window: int):
    """The sections of every file as files of their own: (section mels, their content frames, owner, starts) in file order and
    section order; owner[i] is the file of section i and starts[i] its first frame there.  A section's mel is
    sections.section_mel_ref's bit for bit: its frames, then `window` copies of the file's last column."""
    out, content, owner, starts = [], [], [], []
    for f, (m, c) in enumerate(zip(mels, content_frames)):
        pad = m[:, -1:].expand(-1, window) if c > 0 else None
        for a, b in sections_mod.section_bounds(int(c), cuts[f]):
            out.append(torch.cat([m[:, a:b], pad], dim=1).contiguous())
            content.append(b - a)
            owner.append(f)
            starts.append(a)
    return out, content, owner, starts


def channel_top(mels, content_frames: Optional[Sequence[int]], channel_counts: Sequence[int], options: ChannelOptions,
                window: int = 3000):
    """(top, gated): per recording `top` as uint8 numpy [F] (channels.py, rule 3) and per channel the number of frames the gate
    silenced (rule 4; zero without `bleed_db`) -- channels.channel_top_ref on the device: ONE wm_channel_top call for all
    recordings on the current stream and one copy back.  mels: the channels of all recordings, those of a recording adjacent
    (channel_counts[r] of them, equal in shape and content), contiguous fp16 [n_mels, >= content] on the GPU; with `bleed_db` the
    gated columns are overwritten IN PLACE."""
    n_rec = len(channel_counts)
    if n_rec == 0:
        return [], []
    batch = MelBatch.of(mels, content_frames, "channel_top")
    n_ch, n_mels, dev, content_frames = len(batch), batch.n_mels, batch.device, batch.content_frames
    src, ld, content = batch.rows()
    h, step = options.frames(window, n_mels)
    first = [0]
    for r, c in enumerate(channel_counts):
        mine = range(first[-1], first[-1] + int(c))
        if not 1 <= c <= channels_mod.MAX_CHANNELS or mine.stop > n_ch:
            raise ValueError(f"channel_top: recording {r} has {c} channels (1 .. {channels_mod.MAX_CHANNELS}) of {n_ch} mels")
        if any(batch[i].shape != batch[mine.start].shape or content_frames[i] != content_frames[mine.start] for i in mine):
            raise ValueError(f"channel_top: the channels of recording {r} differ in shape or content")
        first.append(mine.stop)
    if first[-1] != n_ch:
        raise ValueError(f"channel_top: channel_counts {list(channel_counts)} name {first[-1]} of {n_ch} mels")
    frames = [content_frames[first[r]] for r in range(n_rec)]
    total = batch.total
    starts = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    out = torch.empty(int(starts[-1]) + 4 * (n_rec + n_ch) + 8, dtype=torch.uint8, device=dev)       # n_top [n_rec], counts [n_ch], then top
    ints = out[: 4 * (n_rec + n_ch)].view(torch.int32)
    top0 = out.data_ptr() + 4 * (n_rec + n_ch)
    ptrs = torch.tensor([top0 + int(s) for s in starts[:-1]], dtype=torch.int64).to(dev, non_blocking=False)
    first_dev = torch.tensor(first, dtype=torch.int32).to(dev, non_blocking=False)
    lib = native.load_library()
    ws_bytes = int(lib.wm_channel_top_workspace_bytes(n_ch, total))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    native.check(lib.wm_channel_top(src, ld, content, first_dev.data_ptr(), n_rec, n_ch, n_mels, h, step, ptrs.data_ptr(),
                                    ints.data_ptr(), ints[n_rec:].data_ptr(), ws.data_ptr(), ws_bytes, total,
                                    torch.cuda.current_stream(dev).cuda_stream), "wm_channel_top")
    host = out.cpu().numpy()
    head = host[: 4 * (n_rec + n_ch)].view(np.int32)
    if head[:n_rec].tolist() != frames:
        raise ValueError(f"channel_top: wm_channel_top reports {head[:n_rec].tolist()} frames for recordings of {frames}")
    tops = host[4 * (n_rec + n_ch):]
    return [tops[int(a): int(b)].copy() for a, b in zip(starts[:-1], starts[1:])], [int(v) for v in head[n_rec:]]
