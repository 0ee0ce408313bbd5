"""NumPy restatements of the two contracts of speculative greedy decoding (include/eetq_amd.h): the prompt-lookup
draft of eetq_spec_ngram_draft_i64 and the verify / accept / hand-over of eetq_spec_accept_f16.  Written from the contract's
words, loop by loop; nothing here mirrors the kernels' single-pass reduction."""
import numpy as np


def ngram_draft_ref(hist, position, max_ngram, k):
    """hist [B, cols] int64, position an int -> draft [B, k] int64."""
    hist = np.asarray(hist, dtype=np.int64)
    B, cols = hist.shape
    L = min(max(int(position) + 1, 1), cols)
    out = np.zeros((B, k), dtype=np.int64)
    for b in range(B):
        row = hist[b, :L].tolist()
        hit = None
        for n in range(min(max_ngram, L - 1), 0, -1):
            tail = row[L - n:L]
            for e in range(L - 2, n - 2, -1):            # the LARGEST e in [n - 1, L - 2]
                if row[e - n + 1:e + 1] == tail:
                    hit = e
                    break
            if hit is not None:
                break
        if hit is None:
            out[b, :] = row[L - 1]
            continue
        ext = list(row)                                  # the history followed by the draft itself
        for i in range(k):
            ext.append(ext[hit + 1 + i])
        out[b] = ext[L:]
    return out


def greedy_token(row):
    """torch.argmax's answer on an fp16 row: the first index of the maximum, a NaN counts as the maximum, -0 == +0."""
    row = np.asarray(row, dtype=np.float16)
    nan = np.isnan(row)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(row.astype(np.float32)))       # (np.argmax: the first maximum; -0.0 == 0.0 in float compare)


def spec_accept_ref(logits, draft, out_tokens, column, next_token, position, limit, hist, stats):
    """logits [B, k + 1, V] fp16, draft [B, k]; the state arrays are int64 NumPy arrays and ints.  Returns the new
    (out_tokens, column, next_token, position, hist, stats, adv); the inputs are left as they are."""
    logits = np.asarray(logits)
    B, T, _ = logits.shape
    k = T - 1
    out_tokens, hist = np.array(out_tokens, dtype=np.int64), np.array(hist, dtype=np.int64)
    next_token, stats = np.array(next_token, dtype=np.int64), np.array(stats, dtype=np.int64)
    column, position, limit = int(column), int(position), int(limit)
    g = np.array([[greedy_token(logits[b, t]) for t in range(T)] for b in range(B)], dtype=np.int64)
    a = []
    for b in range(B):
        n = 0
        while n < k and draft[b][n] == g[b][n]:
            n += 1
        a.append(n)
    n = min(a)
    adv = max(0, min(min(n + 1, limit - column), k + 1))
    for j in range(adv):
        for b in range(B):
            if 0 <= column + j < out_tokens.shape[1]:
                out_tokens[b, column + j] = g[b, j]
            if 0 <= position + 1 + j < hist.shape[1]:
                hist[b, position + 1 + j] = g[b, j]
    if adv > 0:
        next_token.reshape(B)[:] = g[:, adv - 1]
    stats[0] += 1
    stats[1] += adv
    return out_tokens, column + adv, next_token, position + adv, hist, stats, adv
