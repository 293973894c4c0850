"""A restatement, in plain Python integers, of the two table constructions every HF section depends on (the reference's
entropy.c:267-301 and :184-242; k_build_tables in csrc/hip/kernels.hip; orc_normalize_frequencies and build_alias in
oracle/hyd_oracle.c) that ALSO says which branches a histogram took.

It is the witness of what a picture reaches (tests/entropy_corpus.py, tests/test_entropy_corpus.py) and nothing else:
the GPU is compared with the oracle and with the compiled reference, never with this file.  tests/test_ans_model.py holds
the model itself to the oracle.

normalize(hist) -> (freq, unique, tags); the tags:

  floor_to_1             a count scaled to 0 and was lifted to 1 (the only source of an excess)
  zero_inside            a count of 0 below the alphabet's last token
  deficit                the scaled sum fell short of 4096 and freq[0] took the difference
  deficit_into_empty_f0  ... and token 0 had a count of 0: it gets a frequency without ever being coded
  exact                  the scaled sum was 4096 at once
  excess_partial         the excess loop ended by taking the rest of the excess from an entry larger than it
  excess_flatten         an entry larger than 1 but no larger than the excess was set to 1
  excess_skip            the loop stepped past an entry that was already 1 or 0
  excess_at_0            the scan went down to j = 0 (the partial step took from freq[0])
  unique                 freq[n - 1] == 4096: one symbol owns every slot

alias(freq, log_alphabet_size, unique) -> (cutoff, other, shift, tags); the tags:

  over_to_under          an over-full symbol, after filling an under-full bucket, was left under-full itself
  over_stays             ... was still over-full
  over_lands_exact       ... was left with exactly one bucket
  exact_bucket_initial   a symbol whose frequency is one bucket from the start: on neither list
  pad_under              the alphabet is smaller than the table: empty buckets join the under-full list
  n_eq_table             the alphabet is as large as the table
  unique                 the one-symbol table
"""
ANS_BITS = 12
ANS_SLOTS = 1 << ANS_BITS


def log_alphabet_size(running_max):
    """ceil(log2(running maximum)), at least 5 (entropy.c:952-955)"""
    return max(5, (running_max - 1).bit_length() if running_max > 1 else 0)


def normalize(hist):
    """hist: counts of tokens 0 .. n - 1, the last one non-zero.  -> (freq, unique, tags)"""
    f = [int(v) for v in hist]
    n = len(f)
    assert n and f[-1] > 0 and min(f) >= 0
    tags = set()
    total = sum(f)
    scaled = 0
    for k in range(n):
        if not f[k]:
            if k < n - 1:
                tags.add("zero_inside")
            continue
        v = ((f[k] << ANS_BITS) // total) & 0xFFFF
        if not v:
            v = 1
            tags.add("floor_to_1")
        f[k] = v
        scaled += v
    if scaled == ANS_SLOTS:
        tags.add("exact")
    j = n - 1
    while scaled > ANS_SLOTS:
        assert j >= 0
        excess = scaled - ANS_SLOTS
        if excess < f[j]:
            f[j] -= excess
            scaled -= excess
            tags.add("excess_partial")
            if j == 0:
                tags.add("excess_at_0")
            break
        if f[j] > 1:
            scaled -= f[j] - 1
            f[j] = 1
            tags.add("excess_flatten")
        else:
            tags.add("excess_skip")
        j -= 1
    if scaled < ANS_SLOTS:
        tags.add("deficit")
        if not hist[0]:
            tags.add("deficit_into_empty_f0")
        f[0] += ANS_SLOTS - scaled
    unique = f[n - 1] == ANS_SLOTS
    if unique:
        tags.add("unique")
    assert sum(f) == ANS_SLOTS
    return f, unique, tags


def alias(freq, log_alpha, unique):
    """-> (cutoff, other, shift, tags), each list one entry per bucket of the 2^log_alpha-entry table"""
    n = len(freq)
    table = 1 << log_alpha
    bucket = ANS_SLOTS >> log_alpha
    assert n <= table
    cutoff, other, shift = [0] * table, [0] * table, [0] * table
    tags = set()
    if unique:
        tags.add("unique")
        for i in range(table):
            other[i] = n - 1
            shift[i] = i * bucket
        return cutoff, other, shift, tags
    under, over = [], []
    for s in range(n):
        cutoff[s] = freq[s]
        if freq[s] < bucket:
            under.append(s)
        elif freq[s] > bucket:
            over.append(s)
        else:
            tags.add("exact_bucket_initial")
    tags.add("pad_under" if n < table else "n_eq_table")
    under.extend(range(n, table))
    while over:
        u, o = under.pop(), over.pop()
        cutoff[o] -= bucket - cutoff[u]
        shift[u] = cutoff[o]
        other[u] = o
        if cutoff[o] < bucket:
            under.append(o)
            tags.add("over_to_under")
        elif cutoff[o] > bucket:
            over.append(o)
            tags.add("over_stays")
        else:
            tags.add("over_lands_exact")
    for i in range(table):
        if cutoff[i] == bucket:
            other[i] = i
            cutoff[i] = shift[i] = 0
        else:
            shift[i] -= cutoff[i]  # may be negative: an offset, used only as shift + position
    return cutoff, other, shift, tags


def slots(freq, log_alpha, unique):
    """{(symbol, offset): slot} over all 4096 slots, read in the decoder's direction: slot -> (symbol, offset) must be a
    bijection onto offset < freq[symbol].  -> (map, alias tags)"""
    cutoff, other, shift, tags = alias(freq, log_alpha, unique)
    log_bucket = ANS_BITS - log_alpha
    out = {}
    for slot in range(ANS_SLOTS):
        i, pos = slot >> log_bucket, slot & ((1 << log_bucket) - 1)
        sym, off = (other[i], shift[i] + pos) if pos >= cutoff[i] else (i, pos)
        assert sym < len(freq) and 0 <= off < freq[sym] and (sym, off) not in out, (slot, sym, off)
        out[(sym, off)] = slot
    return out, tags


def histograms(res):
    """raw token counts of every live cluster of one oracle result (binding.LfResult): {cluster: [counts]}, the list
    as long as the cluster's alphabet"""
    out = {}
    for c in range(res.cluster_from, res.cluster_to):
        n = int(res.alphabet_size[c])
        if not n:
            continue
        tok = res.symbols["token"][res.symbols["cluster"] == c]
        h = [0] * n
        for t in tok.tolist():
            h[t] += 1
        out[c] = h
    return out


def witness(res):
    """{cluster: (raw histogram, normalisation tags, alias tags)} of one oracle result; asserts on the way that the model's
    frequencies are the oracle's"""
    out = {}
    for c, h in histograms(res).items():
        f, unique, ntags = normalize(h)
        assert f == [int(v) for v in res.freqs[c][:len(h)]], c
        _, _, _, atags = alias(f, res.log_alphabet_size, unique)
        out[c] = (h, ntags, atags)
    return out


def all_tags(res):
    w = witness(res)
    return set().union(*[n | a for _, n, a in w.values()]) if w else set()
