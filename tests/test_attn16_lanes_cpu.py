"""CPU model of the 16x16-tile attention phase of the fused DiT forward (scldm_amd/csrc/dit_forward.hpp: kM16QK / kM16V, scores16,
the V branch of the attention block; scldm_amd/csrc/dit_aux.hpp: pack_layer_val, m16).  Pure index arithmetic, in the style of
tests/test_mfma16_relayout_cpu.py: this file restates the lane maps of both forms next to the property each step exists for.

The 16x16 form must put every product into the k slot it has in the 32x32 form (two chained 32x32x16 MFMAs = k slots 0..31 in
groups of 8; one 16x16x32 MFMA = the same 32 slots), so that not a bit moves:
  * the packer's row permutation puts head dim d of Q and K into the slot that to_frags_nobias + the 32x32x16 operand map give it;
  * the pair swaps put key kappa of cell c into today's softmax register and today's P V slot, the other cell's keys opposite zeros;
  * the packed output tiles cover AO exactly once, with 8-byte stores that hit every LDS bank once per half wave."""
import itertools

from test_mfma16_relayout_cpu import LANES, XA_LD, HB_LD, cd16, cd32, permlane16_swap, permlane32_swap


# ---- operand maps: which k slot (of the 32 a chained pair / one 16x16x32 covers) element j of a lane's fragment is ----
def slot32(m, lane, j):
    """32x32x16, MFMA m of a chained pair: lane l holds k = 8 (l >> 5) + j of row / col l & 31"""
    return 16 * m + 8 * (lane >> 5) + j


def slot16(lane, j):
    """16x16x32: lane l holds k = 8 (l >> 4) + j of row / col l & 15"""
    return 8 * (lane >> 4) + j


def lane16_of(sp, hh, q):
    return 32 * sp + 16 * hh + q       # the 16x16 form's softmax lane order


def lane32_of(sp, hh, q):
    return 32 * hh + 16 * sp + q       # the 32x32 form's (lane bits 4 and 5 exchanged)


# ---- step 1: the Q / K row permutation ----
def packed_dim(T, r16):
    """pack_layer_val, m16 && kM16QK: row r16 of the head's Q (or K) tile T = this head dim"""
    return 8 * T + 16 * (r16 >> 3) + 4 * ((r16 >> 2) & 1) + (r16 & 3)


def test_row_permutation_is_a_permutation_with_consecutive_quads():
    dims = [packed_dim(T, r) for T in range(2) for r in range(16)]
    assert sorted(dims) == list(range(32))
    # the bias loads: lane group g of tile T reads four consecutive floats at 8 T + 16 (g >> 1) + 4 (g & 1)
    for T, g in itertools.product(range(2), range(4)):
        assert [packed_dim(T, 4 * g + i) for i in range(4)] == [8 * T + 16 * (g >> 1) + 4 * (g & 1) + i for i in range(4)]


def test_head_dims_land_in_todays_k_slots():
    # today: to_frags_nobias packs registers 8 m .. 8 m + 7 of the 32x32 C/D tile (rows = head dims) as operand m of the chained pair
    today = {}
    for lane, m, j in itertools.product(LANES, range(2), range(8)):
        d, tok = cd32(lane, 8 * m + j)
        today.setdefault(tok, {})[slot32(m, lane, j)] = d
    # 16x16 form: pack8(tile 0 registers 0..3, tile 1 registers 0..3) of the two permuted 16-row tiles of a cell
    new = {}
    for lane, e in itertools.product(LANES, range(8)):
        row, tok = cd16(lane, e & 3)
        new.setdefault(tok, {})[slot16(lane, e)] = packed_dim(e >> 2, row)
    for tok in range(16):
        assert sorted(new[tok]) == list(range(32))
        assert new[tok] == today[tok] == today[16 + tok]          # either sample of the shared 32-token tile


def test_qkv_unit_map_covers_every_weight_row_once():
    """pack_layer_val: units 0-31 (Q / K of head u >> 4) and 32-47 (V) of wave w, as gemm_pass16 consumes them: pass-local unit
    v, fragment f = row tile R4 = 2 (v & 1) + f, lane l = row l & 15, k = 32 (v >> 1) + 8 (l >> 4) + j."""
    for w in range(4):
        rows = {}
        for u, f, lane, j in itertools.product(range(48), range(2), LANES, range(8)):
            v = u & 15
            R4, r16, k = 2 * (v & 1) + f, lane & 15, 32 * (v >> 1) + 8 * (lane >> 4) + j
            if u < 32:
                row = (R4 >> 1) * 256 + (w * 2 + (u >> 4)) * 32 + packed_dim(R4 & 1, r16)     # Q rows (R4 0, 1), K rows (2, 3)
            else:
                row = 2 * 256 + w * 64 + 16 * R4 + r16
            rows.setdefault(row, []).append(k)
        want = {p * 256 + w * 64 + r for p in range(3) for r in range(64)}
        assert set(rows) == want
        assert all(sorted(ks) == list(range(256)) for ks in rows.values())


# ---- step 2: scores into the softmax registers ----
def todays_sv(lane, i):
    """32x32 form: sv[i] of a lane = (sample, key, query) of the shared tile's S^T[key][query], own-sample keys only"""
    sp = (lane >> 4) & 1
    key, query = cd32(lane, 8 * sp + i)
    assert key >> 4 == sp == query >> 4
    return sp, key & 15, query & 15


def test_pair_swap_gives_todays_softmax_registers():
    # S^T tiles of the even / odd cell of a pair: element = (cell, key, query)
    S = [[[(c,) + cd16(l, i) for l in LANES] for i in range(4)] for c in range(2)]
    sv = [None] * 8
    for i in range(4):
        sv[i], sv[4 + i] = permlane32_swap(S[0][i], S[1][i])
    for sp, hh, q, i in itertools.product(range(2), range(2), range(16), range(8)):
        assert sv[i][lane16_of(sp, hh, q)] == todays_sv(lane32_of(sp, hh, q), i)


def test_lane_xor_16_exchange_has_todays_operand_order():
    """xor16_sum / xor16_max: swap(v, v) gives (hh = 0's value, hh = 1's value) of the same (sample, query) in both lanes, the
    operand order of xor32_sum / xor32_max in the 32x32 form."""
    v = [((l >> 5, l & 15), (l >> 4) & 1) for l in LANES]          # ((sample, query), hh)
    r0, r1 = permlane16_swap(v, v)
    w = [((((l >> 4) & 1), l & 15), l >> 5) for l in LANES]        # the 32x32 form's lanes
    t0, t1 = permlane32_swap(w, w)
    for l in LANES:
        assert r0[l] == (v[l][0], 0) and r1[l] == (v[l][0], 1)
        assert t0[l] == (w[l][0], 0) and t1[l] == (w[l][0], 1)


# ---- step 3: V operand and P ----
def todays_pv_slots():
    """32x32 form, per (feature, query): slot -> (sample, key) of the V operand, and slot -> (sample, key) or 0 of the P operand.
    V: the swapped pass's C/D tile (rows = tokens) packed as operand m = registers 8 m .. 8 m + 7; P: Ph[m] = the lane's own
    fragment (sv order) where the lane's sample is m, else zero."""
    vslot, pslot = {}, {}
    for lane, m, j in itertools.product(LANES, range(2), range(8)):
        tok, feat = cd32(lane, 8 * m + j)
        vslot.setdefault(feat, {})[slot32(m, lane, j)] = (tok >> 4, tok & 15)
        sp, key, query = todays_sv(lane, j)
        pslot.setdefault((sp, query), {})[slot32(m, lane, j)] = (sp, key) if sp == m else 0
    return vslot, pslot


def test_v_operand_and_p_meet_in_todays_slots():
    vslot, pslot = todays_pv_slots()
    # V tiles of the pair, swapped orientation: register i of lane l = (cell, token 4 (l >> 4) + i, feature l & 15); pack4 gives
    # dwords (i = 0, 1) and (2, 3); one permlane32_swap per dword; Vop dwords = s0[0], s1[0], s0[1], s1[1]
    V = [[[(c,) + cd16(l, i) for l in LANES] for i in range(4)] for c in range(2)]
    s = [permlane32_swap(V[0][i], V[1][i]) for i in range(4)]      # (elements of a dword travel together)
    vop = [s[0][0], s[1][0], s[2][0], s[3][0], s[0][1], s[1][1], s[2][1], s[3][1]]
    new_v = {}
    for lane, e in itertools.product(LANES, range(8)):
        cell, key, feat = vop[e][lane]
        assert feat == lane & 15
        new_v.setdefault(feat, {})[slot16(lane, e)] = (cell, key)
    for feat in range(16):
        assert new_v[feat] == vslot[feat] == vslot[16 + feat]
    # P: lane (sp, hh, q) holds today's own fragment; Ph[m] = own where sp == m else zero, as the B operand of cell m's product
    new_p = {}
    for m, sp, hh, q, j in itertools.product(range(2), range(2), range(2), range(16), range(8)):
        lane = lane16_of(sp, hh, q)
        got = todays_sv(lane32_of(sp, hh, q), j)[:2] if sp == m else 0
        new_p.setdefault((m, q), {})[slot16(lane, j)] = got          # column q of cell m's B operand
        # cell m's product: its own keys opposite its own V, zeros opposite the other cell's V
        vk = new_v[0][slot16(lane, j)]
        assert (got == vk) if sp == m else (got == 0 and vk[0] == sp)
    assert new_p == pslot
    # every query's 16 keys appear exactly once among the non-zero slots of its cell's product
    for m, q in itertools.product(range(2), range(16)):
        keys = [todays_sv(lane32_of(m, hh, q), j)[1] for hh in range(2) for j in range(8)]
        assert sorted(keys) == list(range(16))


# ---- step 4: the AO store ----
def test_ao_store_covers_the_tile_once_and_every_bank_once_per_half_wave():
    """po[R4][cell], lane l: query l & 15 of the cell, head-pair dims 16 R4 + 4 (l >> 4)..+3 (the 16x16 C/D tile of
    mma16(Vop, P): rows = features) -> AO[16 cell + (l & 15)][fbase + 16 R4 + 4 (l >> 4)], one 8-byte store."""
    for ntt in (1, 2):
        seen = {}
        for w, R4, c, lane in itertools.product(range(4), range(4), range(2 * ntt), LANES):
            for i in range(4):
                feat, query = cd16(lane, i)
                row, col = 16 * c + (lane & 15), w * 64 + 16 * R4 + 4 * (lane >> 4) + i
                assert (row, col) == (16 * c + query, w * 64 + 16 * R4 + feat)
                seen[(row, col)] = seen.get((row, col), 0) + 1
        assert set(seen) == set(itertools.product(range(32 * ntt), range(256))) and set(seen.values()) == {1}
    # banks (64 of 4 bytes; an 8-byte store is served 32 lanes at a time): 2-byte elements, row stride XA_LD = 132 dwords = 4 banks
    # mod 64, lane group stride 2 banks - the pattern of the M16 hidden-chunk store on HB_LD (68 dwords)
    for ld, col0 in ((XA_LD, 64 + 16), (HB_LD, 48)):
        for half in range(2):
            banks = []
            for lane in range(32 * half, 32 * half + 32):
                off = 2 * ((16 + (lane & 15)) * ld + col0 + 4 * (lane >> 4))
                assert off % 8 == 0
                banks += [(off // 4) % 64, (off // 4 + 1) % 64]
            assert sorted(banks) == list(range(64))
