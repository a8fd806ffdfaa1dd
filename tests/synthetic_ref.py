"""Pure-Python restatement of gnf_syn_draw (include/gnf_synthetic.h): unbounded ints and masks, independent of numpy's wrapping
arithmetic.  KNOWN_ANSWERS were computed with it once and typed in."""
M64 = (1 << 64) - 1
GOLDEN, M1, M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def mix64(x):
    x ^= x >> 30
    x = (x * M1) & M64
    x ^= x >> 27
    x = (x * M2) & M64
    return x ^ (x >> 31)


def draw(seed, graph, index, stream):
    x = mix64(((seed & M64) + GOLDEN * (graph + 1)) & M64)
    x = mix64(x ^ ((M1 * (index + 1)) & M64))
    x = mix64(x ^ ((M2 * (stream + 1)) & M64))
    return x >> 32


# (seed, graph, index, stream, draw)
KNOWN_ANSWERS = (
    (0, 0, 0, 0, 2378086512),
    (12345, 0, 0, 0, 484917662),
    (12345, 3, 7, 1, 1871851283),
    (12345, 31, 99, 2, 227404947),
    (2 ** 64 - 1, 5, 2 ** 32 - 1, 3, 2667200796),
    (2 ** 63 + 5, 1000, 0, 4, 502174289),
)
