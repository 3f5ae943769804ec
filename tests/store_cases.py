"""The cases the u8 image store is held to, shared by the CPU suite (which proves that the draws of these cases reach the pixels and byte phases that matter) and
the GPU suite (which compares the u8 samplers with their float twins on them).  Nothing here needs a GPU.

Why these: a u8 RGB pixel is 3 bytes at byte offset 3 * (p * H * W + ind) of the store, at any of the four phases of a 4-byte word; the first pixel of the first image
and the last pixel of the last one are where a fetch built from aligned words would leave the store.  5 * 7 * 3 = 105 bytes per image puts the three image bases at
phases 0, 1, 2.  The stores hold every code 0...255 as often as their size allows (q / 255 and q * (1/255) differ for 126 of the 256 codes: test_dataset_cpu.py);
ALL_CODES is one more case, a 16 x 16 image whose uniform draw of 4096 reaches every pixel, and so every code in every channel."""
import numpy as np

SEED = 7
STEPS = (0, 1, 2)
STRIDE, OFFSET = 1, 0
CASES = ((1, 1, 1, 1), (3, 3, 3, 65), (3, 5, 7, 130))                # (P, H, W, N)
WEIGHTED = {2: (1, 4), 4: (1, 7, 16)}                                # error-map grid -> the N of its draws
ALL_CODES = (1, 16, 16, 4096)


def store(P, H, W, C):
    """uint8 [P, H*W, C]: permutations of the 256 codes, one after the other."""
    n = P * H * W * C
    rng = np.random.RandomState(1000 * P + 10 * H + C)
    return np.concatenate([rng.permutation(256) for _ in range(-(-n // 256))])[:n].astype(np.uint8).reshape(P, H * W, C)


def every_code_store(C):
    """uint8 [1, 256, C]: channel c of pixel k holds code (k + 67 c) mod 256 -- every code in every channel."""
    return ((np.arange(256)[:, None] + 67 * np.arange(C)[None, :]) % 256).astype(np.uint8).reshape(1, 256, C)


def poses(P):
    """float32 [P,4,4]: a rotation about y by 0.4 k rad, the camera on a circle of radius 3 -- any pose serves: the twins share it."""
    out = np.zeros((P, 4, 4), dtype=np.float32)
    for k in range(P):
        c, s = np.cos(0.4 * k), np.sin(0.4 * k)
        out[k] = [[c, 0, s, 3 * s], [0, 1, 0, 0.1 * k], [-s, 0, c, 3 * c], [0, 0, 0, 1]]
    return out


def intrinsics(H, W):
    return (1.3 * W, 1.2 * W, W / 2, H / 2)


def error_map(P, G):
    """float32 [P, G*G] of positive weights."""
    return (np.random.RandomState(G).rand(P, G * G) + 0.01).astype(np.float32)
