"""Hotwords and sequence bias by brute force: plain Python loops over one row, written from the contract's words (biasing.py's
docstring) and sharing no code with the product -- numpy is used for the two roundings only (float32 sum, float16 result).

An item is (target, k, prefix, bias): "if the last k tokens of H equal prefix, token target gets bias".  For every token, of the
matching items whose target it is, the one with the greatest k wins, the earlier one in the list at equal k, and its bias is added
once."""
import numpy as np


def bias_row(logits, history, eot, items):
    """`logits`: one row of float16 values (any sequence); `history`: H, the row's sampled tokens.  Returns the new row (float16)."""
    out = np.array(logits, dtype=np.float16).copy()
    H = [int(t) for t in history]
    m = len(H)
    for t in range(min(eot, len(out))):
        best_k, best_bias = -1, None
        for target, k, prefix, bias in items:
            if target != t or k > m:
                continue
            same = True
            for q in range(k):
                if H[m - k + q] != prefix[q]:
                    same = False
                    break
            if same and k > best_k:                  # (strictly greater: at equal k the earlier item stays)
                best_k, best_bias = k, bias
        if best_bias is not None:
            with np.errstate(over="ignore", invalid="ignore"):
                y = np.float32(np.float32(out[t]) + np.float32(best_bias))
                out[t] = np.float16(y)
    return out


def bias_row_sparse(logits, history, eot, items):
    """`bias_row` for a large vocabulary or table: one pass over the items that keeps, per target, the best matching item so far."""
    out = np.array(logits, dtype=np.float16).copy()
    H = [int(t) for t in history]
    m = len(H)
    best = {}
    for target, k, prefix, bias in items:
        if k > m or not 0 <= target < eot:
            continue
        same = True
        for q in range(k):
            if H[m - k + q] != prefix[q]:
                same = False
                break
        if same and (target not in best or k > best[target][0]):
            best[target] = (k, bias)
    for t, (_, bias) in best.items():
        with np.errstate(over="ignore", invalid="ignore"):
            out[t] = np.float16(np.float32(np.float32(out[t]) + np.float32(bias)))
    return out


def bias_batch(logits, tokens, sample_begin, cur_len, eot, items, done=None, row=bias_row_sparse):
    """Row by row over float16 logits [batch, n_vocab] and tokens [batch, >= cur_len]; rows with a `done` flag are copied."""
    out = np.array(logits, dtype=np.float16).copy()
    for b in range(out.shape[0]):
        if done is not None and int(done[b]):
            continue
        out[b] = row(out[b], [int(t) for t in tokens[b][sample_begin:cur_len]], eot, items)
    return out
