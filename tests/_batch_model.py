"""The batches of the batched best-window-per-read pass (csrc/pwm_batch.h) as the GPU tests of its verbs predict
them, so that every one of them can assert that its matrices close batches by both limits."""


def batches(widths):
    """the batches of csrc/pwm_batch.h for these widths: [(number of matrices, why it closed)]"""
    from kmap_amd.device_seq import LIBRARY_BATCH as B, LIBRARY_BATCH_CHUNKS as CH
    out, n, chunks = [], 0, 0
    for w in sorted(widths):
        nch = (w + 3) // 4
        if n == B or chunks + nch > CH:
            out.append((n, "matrices" if n == B else "chunks"))
            n, chunks = 0, 0
        n, chunks = n + 1, chunks + nch
    return out + [(n, "end")]
