"""CPU model of the 16x16-tile GEMM passes of the fused DiT forward (scldm_amd/csrc/dit_forward.hpp: gemm_pass16, relayout16;
scldm_amd/csrc/dit_aux.hpp: pack_layer_val, m16).  Pure index arithmetic: this file restates the lane maps and the unit index
map of the headers next to the property each one exists for.
  * the two lane swaps of relayout16 map the 16x16 MFMA C/D layout onto the 32x32 C/D layout, normal and swapped (V) pass;
  * the unit index map of every moved pass is a bijection onto the pass's (row, k) set, for every wave, the trailing half
    chunk and the zero padding of the hidden dimension included;
  * the B-fragment reads (one ds_read_b128 per 16-token tile) on the padded activation rows: which banks a lane group hits."""
import itertools

import pytest

LANES = range(64)


# ---- lane swaps (v_permlane16_swap_b32 / v_permlane32_swap_b32 without FI / bound control) ----
def permlane16_swap(a, b):
    """odd 16-lane rows of a <-> even 16-lane rows of b"""
    a, b = list(a), list(b)
    for row in (0, 2):
        for i in range(16):
            a[(row + 1) * 16 + i], b[row * 16 + i] = b[row * 16 + i], a[(row + 1) * 16 + i]
    return a, b


def permlane32_swap(a, b):
    """upper 32 lanes of a <-> lower 32 lanes of b"""
    a, b = list(a), list(b)
    for i in range(32):
        a[32 + i], b[i] = b[i], a[32 + i]
    return a, b


def cd16(lane, reg):
    """16x16 C/D: (row, col) held by register reg of a lane"""
    return 4 * (lane >> 4) + reg, lane & 15


def cd32(lane, reg):
    """32x32 C/D: (row, col) held by register reg of a lane"""
    return 8 * (reg >> 2) + 4 * (lane >> 5) + (reg & 3), lane & 31


def relayout16(T0, T1, acc, R):
    """T0 / T1: [reg][lane] of two 16x16 tiles; fills quads 2R, 2R + 1 of acc[reg][lane]"""
    for i in range(4):
        s0, s1 = permlane16_swap(T0[i], T1[i])
        r0, r1 = permlane32_swap(s0, s1)
        acc[(2 * R) * 4 + i] = r0
        acc[(2 * R + 1) * 4 + i] = r1


def tile16(row0, col0):
    """a 16x16 tile whose elements are their own global (row, col)"""
    return [[(row0 + cd16(l, i)[0], col0 + cd16(l, i)[1]) for l in LANES] for i in range(4)]


def test_relayout_maps_the_16x16_layout_onto_the_32x32_layout():
    # normal pass: rows = features, cols = tokens; T0 / T1 = the two 16-token halves of the same 16 rows
    acc = [None] * 16
    for R in range(2):
        relayout16(tile16(16 * R, 0), tile16(16 * R, 16), acc, R)
    for reg, lane in itertools.product(range(16), LANES):
        assert acc[reg][lane] == cd32(lane, reg)


def test_relayout_all_tile_assignment():
    """relayout16_all: t[R4][j] (R4 = the wave's 16-row tile, j = 16-token tile) -> acc[ft][tt], both orientations."""
    for ntt in (1, 2):
        for swap in (False, True):
            # element = (feature row of the wave's 64, token of the workgroup tile)
            def elem(R4, j, lane, reg):
                r, c = cd16(lane, reg)
                return (16 * R4 + c, 16 * j + r) if swap else (16 * R4 + r, 16 * j + c)

            t = [[[[elem(R4, j, l, i) for l in LANES] for i in range(4)] for j in range(2 * ntt)] for R4 in range(4)]
            for ft, tt in itertools.product(range(2), range(ntt)):
                acc = [None] * 16
                for R in range(2):
                    if swap:
                        relayout16(t[2 * ft][2 * tt + R], t[2 * ft + 1][2 * tt + R], acc, R)
                    else:
                        relayout16(t[2 * ft + R][2 * tt], t[2 * ft + R][2 * tt + 1], acc, R)
                for reg, lane in itertools.product(range(16), LANES):
                    r, c = cd32(lane, reg)
                    want = (32 * ft + c, 32 * tt + r) if swap else (32 * ft + r, 32 * tt + c)
                    assert acc[reg][lane] == want


# ---- unit index map (pack_layer_val, m16; consumed by gemm_pass16) ----
H, N_CHUNKS, HC = 684, 5, 128          # the reference DiT's hidden size: 5 chunks of 128 + a half chunk of 64 (684 -> 704)


def unit_elem(v, f, lane, j):
    """pass-local unit v, fragment f, lane, element j -> (row of the wave's 64, k of the pass)"""
    R4 = 2 * (v & 1) + f
    return 16 * R4 + (lane & 15), 32 * (v >> 1) + 8 * (lane >> 4) + j


def pass_elems(units):
    return [unit_elem(v, f, l, j) for v, f, l, j in itertools.product(range(units), range(2), LANES, range(8))]


@pytest.mark.parametrize("units,K", [(16, 256), (8, 128), (4, 64)], ids=["c_proj", "down_chunk", "down_half_chunk"])
def test_unit_map_is_a_bijection_onto_rows_x_k(units, K):
    e = pass_elems(units)
    assert len(e) == 64 * K and set(e) == set(itertools.product(range(64), range(K)))


def test_unit_map_is_what_the_pass_consumes():
    """gemm_pass16: the A operand of mma16 for row tile R4 in k-step ks is fragment R4 & 1 of unit 2 ks + (R4 >> 1); lane l must hold
    row l & 15, k = 8 (l >> 4) .. + 7 of that 16 x 32 block (the 16x16x32 A / B operand map)."""
    for ks, R4, lane, j in itertools.product(range(8), range(4), LANES, range(8)):
        assert unit_elem(2 * ks + (R4 >> 1), R4 & 1, lane, j) == (16 * R4 + (lane & 15), 32 * ks + 8 * (lane >> 4) + j)


def test_weight_rows_and_hidden_padding_per_wave():
    rows_proj, rows_down = set(), set()
    for w in range(4):
        for v, f, l in itertools.product(range(16), range(2), LANES):
            rows_proj.add(w * 64 + unit_elem(v, f, l, 0)[0])             # attn.c_proj.weight row
        for v, f, l in itertools.product(range(8), range(2), LANES):
            rows_down.add(w * 64 + unit_elem(v, f, l, 0)[0])             # mlp.c_proj.weight row
    assert rows_proj == set(range(256)) and rows_down == set(range(256))
    # hidden index of the down-projection: chunk c covers c*128 .. +127, the half chunk 640 .. 703; hid >= H is exact zero padding
    hid = []
    for c in range(N_CHUNKS):
        hid += [c * HC + k for (r, k) in pass_elems(8) if r == 0]
    half = [N_CHUNKS * HC + k for (r, k) in pass_elems(4) if r == 0]
    assert sorted(hid + half) == list(range(704))
    padded = [h for h in half if h >= H]
    assert sorted(padded) == list(range(684, 704)) and all(h < H for h in hid)


# ---- B-fragment reads: one ds_read_b128 per 16-token tile at (l & 15) * ld + (l >> 4) * 8 elements (2-byte elements) ----
B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS]
XA_LD, HB_LD = 256 + 8, 128 + 8        # FwdLayout: 16 bytes of row pad


@pytest.mark.parametrize("ld,ksteps", [(XA_LD, 8), (HB_LD, 4)], ids=["XA", "HB"])
def test_b_fragment_reads_bank_pattern(ld, ksteps):
    """The row stride is 4 banks (mod 64), the k-group stride 4 banks: rows r and r + 1 of k-group g and g + 1 share a 16-byte slot.
    The hardware's ds_read_b128 lane groups are not the 16-lane rows, so inside each group exactly ONE slot is hit by two lanes
    (5 LDS cycles instead of 4 per read), the other 14 once - the same pattern gemm_pass_tile16 has always read with."""
    for j, ks in itertools.product(range(4), range(ksteps)):
        for group in B128_GROUPS:
            slots = {}
            for lane in group:
                off = 2 * ((j * 16 + (lane & 15)) * ld + (lane >> 4) * 8 + ks * 32)
                assert off % 16 == 0
                slots.setdefault((off >> 4) % 16, set()).add(off)
            ways = sorted(len(a) for a in slots.values())
            assert ways == [1] * 14 + [2]
