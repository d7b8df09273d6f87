"""Operand lists of the field-layer tests, shared by the GPU comparisons
(test_gpu_primitives.py, test_gpu_field_products.py) and by the CPU check that the lists reach the
rare carry paths of the device's products (test_ec_model.py)."""
from ec_model import M256, P
from helpers import rng

# op name -> (praos_debug_fe_multi code, products M, squaring)
MULTI_OPS = {"fe_mul2": (0, 2, False), "fe_sq2": (1, 2, True), "fe_mul3": (2, 3, False),
             "fe_mul4": (3, 4, False), "fe_sq4": (4, 4, True)}
ALIASED = 8


def edge_values():
    v = [0, 1, 2, 19, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 ** 255 - 1, 2 ** 255, 2 ** 256 - 1, 2 ** 256 - 38,
         2 ** 256 - 39, 38, 2 ** 32 - 1, 2 ** 224]
    return [x % 2 ** 256 for x in v]


def rare_fold_pairs():
    """(op, x, y) pairs whose second 2^256 fold carries (add, mul) or borrows (sub) out of limb 0,
    the branch fe25519.hpp takes with probability < 2^-21 on random operands (PRAOS_RED_BRANCH)."""
    m = 2 ** 256
    pairs = [("add", m - 1, 2 ** 32 - 9), ("add", m - 1, m - 9), ("add", m - 1, m - 1),
             ("add", m - 38, m - 1), ("sub", 3, 2 ** 32), ("sub", 0, m - 5), ("sub", 37, m - 1),
             ("sub", 0, 1), ("sub", 0, m - 1)]
    # (2^256 - 1) b folds to 37 b - 38 (b < 2^256 / 37): limb 0 = 2^32 - 1 for b = 2^32 j + 1, and
    # 37 b - 38 >= 2^256 - 38 (the carry runs through every limb) for b = ceil(2^256 / 37)
    pairs += [("mul", m - 1, 2 ** 32 * j + 1) for j in (1, 2, 3, 2 ** 64, 2 ** 190)]
    pairs += [("mul", m - 1, -(-m // 37)), ("mul", -(-m // 37), m - 1)]
    return pairs


def rare_mul_pairs():
    return [(x, y) for o, x, y in rare_fold_pairs() if o == "mul"]


def rare_squares():
    """a = 2^256 - x, x <= 30: a^2 folds to 37 2^256 + (2^256 - (76 x - x^2)), every limb above limb 0
    all-ones and limb 0 within 38 * 37 of 2^32: the second fold's carry runs through every limb."""
    return [M256 - x for x in (1, 2, 3, 29, 30)]


def structured_values():
    """All-ones limbs, one all-ones limb at each position, alternating 0 / 0xFFFFFFFF limbs, and
    2^256 - 76, 2^256 - 77: (2^256 - x)(2^256 - y) = 2^512 - (x + y) 2^256 + x y has first fold
    38 2^256 + x y - 38 (x + y), so these two (and their squares) give k = 38, the largest k there is."""
    single = [(2 ** 32 - 1) << (32 * i) for i in range(8)]
    even = sum(single[0::2])
    odd = sum(single[1::2])
    return [M256 - 1] + single + [even, odd, M256 - 76, M256 - 77]


def ring_pairs(seed=1, n=400):
    """Operand pairs of the single-product tests: the full cross product of the edge values, then
    n random pairs (the random tail test_fe_ring_ops always had)."""
    e = edge_values()
    r = rng(seed)
    xs = [r.getrandbits(256) for _ in range(n)]
    ys = [r.getrandbits(256) for _ in range(n)]
    return [(x, y) for x in e for y in e] + list(zip(xs, ys))


def product_pairs():
    """Operand pairs every slot of every interleaved product sees."""
    e, s = edge_values(), structured_values()
    r = rng(11)
    rnd = [(r.getrandbits(256), r.getrandbits(256)) for _ in range(300)]
    return [(x, y) for x in e for y in e] + [(x, y) for x in s for y in s] + rnd


def multi_lanes(name):
    """Lanes of one praos_debug_fe_multi op: a list of M (a, b) pairs per lane (b unused by the
    squarings).  Every slot sees the whole of product_pairs() (slot m is the list rotated by m
    strides, so the products of a lane are unrelated); then each rare-fold case stands in each
    slot in turn while the other slots hold random values."""
    _, M, square = MULTI_OPS[name]
    pairs = product_pairs()
    n = len(pairs)
    step = n // M + 1
    lanes = [[pairs[(i + m * step) % n] for m in range(M)] for i in range(n)]
    rare = [(a, a) for a in rare_squares()] if square else rare_mul_pairs()
    r = rng(12)
    for pr in rare:
        for m in range(M):
            lane = [(r.getrandbits(256), r.getrandbits(256)) for _ in range(M)]
            lane[m] = pr
            lanes.append(lane)
    return lanes


def weak_values():
    """Inputs of the unary field tests: edge values x, x + p and x + 2p where below 2^256,
    and the neighbours of 0, p and 2p."""
    v = list(edge_values())
    for x in edge_values():
        for k in (1, 2):
            if x + k * P < M256:
                v.append(x + k * P)
    v += [0, P, 2 * P, P - 1, P + 1, 2 * P - 1, 2 * P + 1]
    r = rng(13)
    v += [r.getrandbits(256) for _ in range(100)]
    return v
