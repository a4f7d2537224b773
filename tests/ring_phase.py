"""Cases and seeded inputs of tests/test_ring_phase_cpu.py and tests/test_gpu_ring_phase.py.

The two dense MFMA kernels read their operands from a ring of LDS stage buffers (three in csrc/wino_mfma.hip, two in
csrc/fc_mfma.hip) and carry the ring position in the `offset:` field of every ds_read_b128. Which buffer a read
addresses depends on the number of 64-deep K stages per plane (trunk) or per split-K slice (fc) modulo the ring
length. The case lists of tests/exact.py only have Cin in {64, 128, 256, 512} — 1, 2, 4 or 8 stages, or their halves
under the Cin split — and fc K that are multiples of 128: never a stage count that is 0 (mod 3), never an odd one above 1.
These cases add them, at the smallest shapes that still fill a workgroup partially and, for the grouped ones, take
more than one. Everything is exact-integer data (tests/exact.py): the kernel must equal float64 bit for bit, so a
read from the wrong buffer cannot pass.
"""
import exact

# ((B, H, W, Cin), Cout, pool, groups), the Cin split S the library must report, stages per plane and slice = Cin / 64 / S
TRUNK_CASES = [
    (((1, 8, 12, 64), 64, 0, 1), 1, 1),      # one partially filled workgroup: 6 tiles, 26 clamped rows
    (((1, 8, 12, 128), 64, 0, 1), 2, 1),
    (((1, 8, 12, 192), 64, 0, 1), 1, 3),     # a plane is one full turn of the ring
    (((1, 8, 12, 320), 64, 0, 1), 1, 5),
    (((1, 8, 12, 448), 64, 0, 1), 1, 7),
    (((2, 12, 20, 192), 128, 1, 2), 1, 3),   # two filter sets, two channel blocks, pooled output only
    (((2, 12, 20, 320), 64, 2, 2), 1, 5),    # ... both outputs
    (((1, 8, 12, 384), 64, 0, 1), 2, 3),     # the Cin split (the op hands the workspace over): 3 stages per slice
]

# (capacity, K, N) of ops.fc_rows, each over exact.fc_counts(capacity)
FC_CASES = [
    (64, 192, 64),      # 3 stages
    (130, 320, 128),    # 5 stages, three row blocks, two column blocks
    (64, 1088, 64),     # 17 stages; one live block: the device splits K in 2 — slices of 8 and 9 stages
    (64, 1728, 64),     # 27 stages; split in 3 — slices of 9 stages from stage 0, 9 (odd) and 18
]
FC_COLS_CASE = (70, 192, 88, 128)    # fc_rows_cols: capacity, K, out_features, padded
FC_SPLIT_CASE = (70, 192, 64, 64)    # fc_rows_split: capacity, K, out_a, out_b


def trunk_inputs(case, device=None):
    return exact.wino_inputs(case, device)


def fc_inputs(cap, K, N, device=None):
    """x [cap, K], wt [N, K] integers in [-FC_A, FC_A], bias [N] in [-FC_BIAS, FC_BIAS]."""
    s = exact.seed_of("ring_phase fc", cap, K, N)
    return (exact.ints(s, (cap, K), -exact.FC_A, exact.FC_A, device=device), exact.ints(s + 1, (N, K), -exact.FC_A, exact.FC_A, device=device),
            exact.ints(s + 2, (N,), -exact.FC_BIAS, exact.FC_BIAS, device=device))


def fc_shapes():
    """Every (capacity, K, N) the GPU file runs, the padded / two-layer ones at the width their products have."""
    cap_c, K_c, N_c, _ = FC_COLS_CASE
    cap_s, K_s, a, b = FC_SPLIT_CASE
    return list(FC_CASES) + [(cap_c, K_c, N_c), (cap_s, K_s, a + b)]
