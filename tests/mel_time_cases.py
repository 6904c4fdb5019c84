"""Shapes of the time-parallel upsampling tests and a numpy mirror of what mel_time_upsample_kernel and its host
side rely on: which frames a sample range reads, how many MFMA columns a call has, and which variant of the kernel the host takes
for them."""
import condgen

# (window, stride) of the prime tests' shape; 48 / 16 is one frame per time tile
PRIME_HOPS = [(8, 2), (12, 4), (16, 8), (48, 16)]
PRIME_LENGTHS = (1, 2, 15, 16, 17, 40, 47)
LONG_HOP, LONG_LENGTHS = (16, 8), (100, 300)
C1_HOP256_LENGTHS = (255, 256, 257, 600)
OTHER_R_HOP, OTHER_R_LENGTHS = (12, 4), (17, 47)
SCORE_LENGTHS = (1, 16, 17, 47)

# the conditioning cases whose rows are held to the lockstep upsampling
ROW_CASES = ["cond_C3_B16", "cond_C3_B21_n37", "cond_oddL_B19", "cond_C1_B1"]
assert all(n in condgen.COND_BY_NAME for n in ROW_CASES)

# frames per utterance at the real hops: (stride + 1, 2 stride + 3) ends in the fourth frame
HOP_FRAMES = 5
# launchMelTime: up to this many groups of 16 columns the operand is read from L2 (a group per blockIdx.y, the phases spread over
# about 1024 workgroups of four waves), above it from LDS (a phase per workgroup, at most 1024 of them)
DIRECT_GROUPS, WAVES, GRID = 4, 4, 1024


def frames_read(a, b, window, stride):
    """(first, last) frame read for the samples [a, b): max(0, a / stride - (m - 1)) .. (b - 1) / stride, m = window / stride."""
    assert 0 <= a < b and window % stride == 0
    m = window // stride
    return max(0, a // stride - (m - 1)), (b - 1) // stride


def ranges(N, stride):
    """(first_sample, count) of one call's requests, ranges that cut frames: the whole utterance, sample 1 alone, across the first
    frame edge, from inside the second frame into the fourth, a start that is a multiple of 16 and (where a stride allows it: not
    2, 4, 8 or 16) not of the stride, the last sample alone.  N must hold them all."""
    sixteen = next((t for t in range(16, N, 16) if t % stride), 16)
    out = [(0, N), (1, 1), (stride - 1, 2), (stride + 1, 2 * stride + 3), (sixteen, min(N - sixteen, stride + 5)), (N - 1, 1)]
    assert all(a >= 0 and c >= 1 and a + c <= N for a, c in out), (N, stride, out)
    return out


def columns(reqs, stride):
    """MFMA columns of a call: the frames a / stride .. (b - 1) / stride of every request (first_sample, count)"""
    return sum((a + c - 1) // stride - a // stride + 1 for a, c in reqs)


def plan(reqs, stride):
    """(variant, passes): which kernel the host launches for the call -- "l2" or "lds" -- and how often the busiest workgroup (l2:
    wave) goes round its phase loop"""
    groups = -(-columns(reqs, stride) // 16)
    if groups <= DIRECT_GROUPS:
        gx = min(-(-stride // WAVES), -(-GRID // groups))
        return "l2", -(-stride // (gx * WAVES))
    return "lds", -(-stride // min(stride, GRID))
