"""The one restatement, for the tests, of how csrc/attn32.hip widens a key-block range of kvq_attn32_key_ranges to a body it holds."""
KB = 13                     # 32-key blocks of the LDS images
BODY_LENGTHS = (4, 7, 13)   # key blocks per inlined q-block body of the ranges kernel


def widened(first, last):
    """(t0, length) of the key blocks [t0, t0 + length) the kernel runs for the range [first, last]: the shortest body that holds the
    range, moved down where it would pass block 12"""
    need = last - first + 1
    length = next(n for n in BODY_LENGTHS if need <= n)
    return min(first, KB - length), length
