"""NumPy restatement of the contract of eetq_spec_sample_accept_f16 (include/eetq_amd.h), written from the
contract's words, loop by loop: the draw of every verify row (tests/sampling_ref.py: float64 sampling, the greedy rule, Philox),
the walk with EOS flags and objections, the hand-over.  A plain module for the tests (not a conftest)."""
import numpy as np

import sampling_ref


def draw_tokens(logits, column, want, temperature=0.0, top_k=0, top_p=1.0, seed=0, uniforms=None):
    """Step 1: x[b][t] for t < want (-1 beyond: those positions are not read)."""
    logits = np.asarray(logits)
    B, T, _ = logits.shape
    x = np.full((B, T), -1, dtype=np.int64)
    sampled = temperature > 0                                         # 0, negative and NaN select greedy
    for b in range(B):
        for t in range(want):
            if not sampled:
                x[b, t] = sampling_ref.greedy_token(logits[b, t])
                continue
            if uniforms is None:
                u = sampling_ref.philox_uniform(seed, column + t, b)
            else:
                u = np.float32(uniforms[b][t])
                u = np.float32(0.0) if not u > 0 else np.float32(1.0 - 2.0 ** -24) if u >= 1 else u
            u = np.floor(np.float64(u) * 2.0 ** 24) / 2.0 ** 24       # the entry uses u in steps of 2^-24
            x[b, t] = sampling_ref.sample_row(logits[b, t], temperature, top_k=top_k, top_p=top_p).token(u)
    return x


def spec_sample_accept_ref(x, draft, out_tokens, column, next_token, position, limit, hist, stats, eos_token=-1, pad_token=0,
                           done=None):
    """Steps 2 and 3 on drawn tokens x [B, k + 1] (``draw_tokens``, or any oracle of step 1); draft [B, k]; the state arrays
    are int64 NumPy arrays and ints, done an int array [B] or None.  Returns the new (out_tokens, column, next_token, position,
    hist, stats, done, adv); the inputs are left as they are."""
    x, draft = np.asarray(x, dtype=np.int64), np.asarray(draft, dtype=np.int64)
    B, T = x.shape
    k = T - 1
    out_tokens, hist = np.array(out_tokens, dtype=np.int64), np.array(hist, dtype=np.int64)
    next_token, stats = np.array(next_token, dtype=np.int64), np.array(stats, dtype=np.int64)
    done_out = None if done is None else np.array(done, dtype=np.int32)
    column, position, limit = int(column), int(position), int(limit)
    want = max(0, min(limit - column, k + 1))
    # 2. the walk
    fin = [False] * B if done is None else [bool(d) for d in done]
    y = np.zeros((B, T), dtype=np.int64)
    fin_at = np.zeros((B, T), dtype=bool)                             # fin_b after position t
    adv = want
    for t in range(want):
        objects = False
        for b in range(B):
            y[b, t] = pad_token if fin[b] else x[b, t]
            if eos_token >= 0 and y[b, t] == eos_token:
                fin[b] = True
            fin_at[b, t] = fin[b]
            if t < k and not fin[b] and draft[b, t] != y[b, t]:
                objects = True
        if objects:
            adv = t + 1
            break
    # 3. the hand-over
    for j in range(adv):
        for b in range(B):
            if 0 <= column + j < out_tokens.shape[1]:
                out_tokens[b, column + j] = y[b, j]
            if 0 <= position + 1 + j < hist.shape[1]:
                hist[b, position + 1 + j] = y[b, j]
    if adv > 0:
        next_token.reshape(B)[:] = y[:, adv - 1]
        if done_out is not None:
            done_out[:] = fin_at[:, adv - 1]
    stats[0] += 1
    stats[1] += adv
    return out_tokens, column + adv, next_token, position + adv, hist, stats, done_out, adv
