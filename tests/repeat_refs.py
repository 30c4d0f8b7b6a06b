"""Repetition penalty and no-repeat n-grams by brute force: plain Python loops over one row, written from the contract's words
(repetition.py's docstring) and sharing no code with the product's vectorised statements -- numpy is used for the two roundings only
(float32 arithmetic, float16 result)."""
import numpy as np


def controls_row(logits, history, eot, p, n):
    """`logits`: one row of float16 values (any sequence); `history`: H, the row's sampled tokens.  Returns the new row (float16)."""
    out = np.array(logits, dtype=np.float16).copy()
    H = [int(t) for t in history]
    m = len(H)
    p32 = np.float32(p)
    # the penalty: every distinct text token once
    if p32 != np.float32(1.0):
        seen = []
        for t in H:
            if t >= eot or t in seen:
                continue
            seen.append(t)
            x = np.float32(out[t])
            with np.errstate(over="ignore", invalid="ignore"):
                y = np.float32(x / p32) if x > 0 else np.float32(x * p32)
                out[t] = np.float16(y)
    # the bans: every earlier (n - 1)-gram equal to the last n - 1 tokens bans the token that followed it
    if n > 0 and m >= n - 1:
        suffix = H[m - (n - 1):] if n > 1 else []
        for i in range(0, m - n + 1):
            gram = [H[i + k] for k in range(n - 1)]
            if gram == suffix:
                t = H[i + n - 1]
                if t < eot:
                    out[t] = np.float16(-np.inf)
    return out


def controls_batch(logits, tokens, sample_begin, cur_len, eot, p, n, done=None):
    """Row by row over float16 logits [batch, n_vocab] and tokens [batch, >= cur_len]; rows with a `done` flag are copied."""
    out = np.array(logits, dtype=np.float16).copy()
    for b in range(out.shape[0]):
        if done is not None and int(done[b]):
            continue
        out[b] = controls_row(out[b], [int(t) for t in tokens[b][sample_begin:cur_len]], eot, p, n)
    return out


def has_repeated_ngram(seq, n, eot):
    """Does `seq` hold two n-grams that are equal and end in a text token (the thing no_repeat_ngram_size = n forbids)?"""
    seen = set()
    for i in range(len(seq) - n + 1):
        gram = tuple(int(t) for t in seq[i:i + n])
        if gram[-1] < eot:
            if gram in seen:
                return True
        seen.add(gram)
    return False
