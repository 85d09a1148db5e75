// The layout of the tables the LDPC plan (k_ldpc.hip) builds for the fast kernels (k_ldpc_wg8.hip, k_ldpc_cu1.hip, k_ldpc_lat.hip, k_ldpc_nat.hip) and
// tools/plan_probe.cpp reads back: ONE place for every dword index, field and sentinel.  Constants are usable from host and device; the kernels use the
// constants alone (a helper function in front of an expression can move an instruction of the 27-slot layer loop); the pack / unpack helpers are host code.
//
// LdpcPlan::w8_tab = LdpcKParams::w8.tab
//   [q][LDPC_FAST_STRIDE]        one LAYER TABLE of 64 dwords per layer:
//        0 .. 26                   the slots' entries (fast_deg of them), see "entry"
//        LT_PRIM        (27)       mask of the primary slots (no duplicate edge of a bit-group in front of them in the layer, not NULL)
//        LT_CINFO       (28)       conflict info: ncf | slot of conflict entry 0 << 8 | its level << 13 | slot of entry 1 << 16 | its level << 21
//        LT_CONF0, 1    (29, 30)   conflict entries 0 and 1 once more (one scalar load brings 27 .. 31)
//        LT_DUPMASK     (31)       mask of the slots with a duplicate edge
//        LT_CONF + i    (32 ..)    the conflict entries (duplicate edges sorted by level, then slot), at most LDPC_FAST_MAXC = 16
//        LT_CONF_META + i (48 ..)  slot | level << 8 of conflict entry i
//        LDPC_TANH_ORDER + k (56 .. 60)  sum-product plans (at most LDPC_SPA_MAXC conflict entries, so the meta words end below 56): the slots in the ORACLE's edge
//                                  order, LT_ORDER_BITS bits each, LT_ORDER_PER_DWORD per dword
//   modes 4 / 5 / 6, behind the q layer tables:
//        [q][NR] dwords            the row-keeping waves' swaps: the LDS position register slot k swaps with during layer r, LT_SWAP_NONE = none
//        modes 4 / 5: [q][lo, hi]  the same as one 64-bit mask per layer: bit k = slot k swaps with LDS position k during layer r
//        mode 6: [q][2 groups][lo, hi]  per group of row-keeping waves: bit k = slot k of the group swaps with its position (= its index)
//
// entry: byte shift 4 t0 (11 bits) | byte offset of the bit-group's row in its store (18 bits) << 11 | LDS flag << 29.
//
// LdpcPlan::w8_rows = LdpcKParams::w8.rows, sections in this order:
//        [w8_nl]                   bit-group of LDS row l (parked modes: of the row at position l at the start of an iteration)
//        [w8_ng]                   bit-group of global row l
//        [q]                       where parity group r lives: byte offset of its row in LDS, or ROWS_GLOBAL (bit 31) | byte offset inside the workgroup's global
//                                  slot; mode 6: byte offset of its LDS position at the start of an iteration, or ROWS_NONE = it starts in a register slot
//        [NR] (parked modes)       bit-group in register slot k at the start of an iteration, ROWS_NONE = empty
//
// LdpcPlan::nat_tab (k_ldpc_nat.hip): [q][fast_deg][2] = { t0 (NAT_T0_MASK) | NAT_PARITY | NAT_NULL, first bit of the group }.
//
// Left as they are on purpose: the kernels find the swap sections with their own expression, `tab + q * LDPC_FAST_STRIDE (+ q * NR)` (k_ldpc_wg8.hip w8_park_server,
// k_ldpc_cu1.hip cu1_keeper) -- it is lt_swaps_at / lt_swap_masks_at written out, with the named stride and the kernel's compile-time NR; a helper call there is
// what device code avoids (see above).  A change of the sections' order has to be made there too.
//
// LdpcPlan::w8_atab: per-lane addresses; ATAB_DROPPED is an offset every buffer access drops (idle lanes, padding slots).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dvbs2 {

constexpr int LDPC_FAST_STRIDE = 64;   // dwords per layer table
constexpr int LDPC_TANH_ORDER = 56;    // first dword of the sum-product plans' edge order

enum : int {
    LT_PRIM = 27, LT_CINFO = 28, LT_CONF0 = 29, LT_CONF1 = 30, LT_DUPMASK = 31, LT_CONF = 32, LT_CONF_META = 48,
    LT_BASE_SHIFT = 11, LT_LDS_SHIFT = 29,                                      // entry
    LT_CINFO_SLOT0_SHIFT = 8, LT_CINFO_LVL0_SHIFT = 13, LT_CINFO_SLOT1_SHIFT = 16, LT_CINFO_LVL1_SHIFT = 21,
    LT_META_LVL_SHIFT = 8,
    LT_ORDER_BITS = 5, LT_ORDER_PER_DWORD = 6,
    ROWS_GLOBAL_BIT = 31,
    NAT_PARITY_BIT = 16, NAT_NULL_BIT = 17,
};
enum : uint32_t {
    LT_SHIFT_MASK = 0x7FFu, LT_BASE_MASK = 0x3FFFFu, LT_LDS = 1u << LT_LDS_SHIFT,
    LT_CINFO_NCF_MASK = 0xFFu, LT_SLOT_MASK = 31u, LT_LVL_MASK = 3u,
    LT_SWAP_NONE = 0xFFu,
    ROWS_NONE = 0xFFFFFFFFu, ROWS_GLOBAL = 1u << ROWS_GLOBAL_BIT,
    NAT_T0_MASK = 0xFFFFu, NAT_PARITY = 1u << NAT_PARITY_BIT, NAT_NULL = 1u << NAT_NULL_BIT,
    ATAB_DROPPED = 0x7FFFF000u,
};

// ---- host side: the plan packs, the probe unpacks
inline uint32_t lt_pack_entry(uint32_t shift_bytes, uint32_t base_bytes, bool lds) { return shift_bytes | (base_bytes << LT_BASE_SHIFT) | (lds ? (uint32_t)LT_LDS : 0u); }
inline uint32_t lt_shift(uint32_t e) { return e & LT_SHIFT_MASK; }
inline uint32_t lt_base(uint32_t e) { return (e >> LT_BASE_SHIFT) & LT_BASE_MASK; }
inline bool lt_is_lds(uint32_t e) { return ((e >> LT_LDS_SHIFT) & 1u) != 0u; }
inline uint32_t lt_pack_meta(uint32_t slot, uint32_t lvl) { return slot | (lvl << LT_META_LVL_SHIFT); }
inline uint32_t lt_meta_slot(uint32_t m) { return m & LT_SLOT_MASK; }
inline uint32_t lt_meta_lvl(uint32_t m) { return m >> LT_META_LVL_SHIFT; }
inline uint32_t lt_ncf(uint32_t cinfo) { return cinfo & LT_CINFO_NCF_MASK; }
// conflict entry i (0 or 1) of a layer in the info word: its slot and its level, where the kernels unpack them
inline uint32_t lt_cinfo_field(uint32_t meta, int i)
{
    return i == 0 ? (lt_meta_slot(meta) << LT_CINFO_SLOT0_SHIFT) | (lt_meta_lvl(meta) << LT_CINFO_LVL0_SHIFT)
                  : (lt_meta_slot(meta) << LT_CINFO_SLOT1_SHIFT) | (lt_meta_lvl(meta) << LT_CINFO_LVL1_SHIFT);
}
// where the swap masks start behind the q layer tables and the [q][NR] swap dwords
inline size_t lt_swaps_at(int q) { return (size_t)q * LDPC_FAST_STRIDE; }
inline size_t lt_swap_masks_at(int q, int NR) { return lt_swaps_at(q) + (size_t)q * NR; }

}  // namespace dvbs2
