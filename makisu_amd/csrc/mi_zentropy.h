// mi_zentropy.h -- the host side of the zpack entropy stage (mi_zentropy.hip), for the translation units whose readers must
// accept form H (mi_zpack.hip: the decode into a plain blob and MI_ZPACK_VERIFY; mi_zset.hip: the fused restore; mi_zrecode.hip:
// the recode's decode and recheck) and for the ones that code it (mi_zpack.hip: mi_pack_compress; mi_zrecode.hip).  Host types only.
#pragma once
#include "mi_internal.h"
#include "mi_local.h"
#include "host_huff.h"

namespace mi {

// THE UNWRAP PRE-PASS over a reader's row arrays ON THE DEVICE, which it rewrites: row k's stored span lies at base +
// d_src[k * src_stride] and its length | stored << 32 word at d_word[k * word_stride] (a zpack's rows: the offset and length words
// of its 56-byte entries, strides 7, base = the blob; a restore's rows: addresses and words, strides 1, base 0).  The arrays are
// the CALL'S OWN COPIES: nothing a set or a zpack keeps is written.  run():
//   classify   one launch; the counts and stored bytes per form come to the host (one synchronisation).  No form H: nothing
//              else is allocated or launched, the arrays are as they were, every result is as before there was a stage;
//   unwrap     else mi_plan.h's scan over the inner lengths, ONE scratch for the inner forms (it does not fit: MI_ERR_NOMEM
//              naming its size under `who`, nothing has changed), zh_unwrap_kernel one wave a row.  A row that unwraps is
//              rewritten to point at its inner form (kind 1: an LZ4 row of the inner length; kind 2: a raw row); a refused row
//              stays as it was -- the LZ4 decoder refuses its 0x00 token too -- and its rule (8..11, or 7 for the pad behind the
//              span) is kept.  Blocking on the ctx stream.
// The caller then runs its LZ4 kernel over the arrays WHILE THIS OBJECT LIVES (the scratch is its member) and hands what that
// kernel found to merge(): the smallest refused row of both passes and its rule, in host_huff.h's order (8..11 before the inner
// block's 1..6 before 7).
struct MI_LOCAL ZhUnwrap {
    DevBuf inner, aux, cells;
    mi_zforms forms = {};
    u64 n_h = 0, bad = ~0ull, inner_bytes = 0, n_rows = 0;
    u32 rule = 0;
    int run(mi_ctx* c, const char* who, u64 base, u64* d_src, u32 src_stride, u64* d_word, u32 word_stride, u64 n);
    // on the device, row k's rule at k (0: none); NULL where no form H was met
    const u32* rules() const { return n_h ? (const u32*)(aux.as<u64>() + n_rows) : nullptr; }
    void merge(u64* lz_bad, u32* lz_rule) const {
        if (bad == ~0ull || (*lz_bad != ~0ull && *lz_bad < bad)) return;
        if (*lz_bad == bad && rule == mi_host::kLz4PadNotZero && *lz_rule != 0) return;      // the inner block's rule comes first
        *lz_bad = bad;
        *lz_rule = rule;
    }
};

// the counts alone (mi_zpack_count_forms, mi_zset_count_forms): the classify launch over arrays that are only read; d_tags (may
// be NULL): row k counts only if d_tags[k] != 0 -- a set's table.  Blocking
MI_LOCAL int zh_count_forms(mi_ctx* c, u64 base, const u64* d_src, u32 src_stride, const u64* d_word, u32 word_stride, u64 n, const u64* d_tags,
                            mi_zforms* out);

// MI_ZPACK_ENTROPY behind a coder's encode kernel, ENQUEUED on the ctx stream: one wave a row of d_rows (the offset word counts
// from d_base, the stored size is the coder's), the form under it in d_scratch at d_woff[k] or, raw, in the pack; a kept form H
// goes to d_scratch2 at d_woff[k], the row's stored size becomes its size and d_hsrc[k] its device address (else 0)
MI_LOCAL void zh_encode_enqueue(mi_ctx* c, const void* d_base, u64* d_rows, const u64* d_woff, const void* d_scratch, void* d_scratch2,
                                u64* d_hsrc, u64 n, u32 waves);
// mi_zset_recode with the stage (mi_zrecode.hip), each ENQUEUED on the ctx stream between that file's own kernels: the unwrap's
// rules merged into a round's per-row rules; form H over a round's candidates (u_src, u_word: the unwrapped rows, r_off: the rows'
// places in the round's scratch, scratch2: as large; r_cand[k] becomes the size of a kept form, which then lies where the coder's
// candidate lay); the recheck's rows (entry i of the list of replaced rows) and its decode of unwrapped rows, raw ones among them
MI_LOCAL void zh_rules_merge_enqueue(mi_ctx* c, const u32* h_rule, u32* r_rule, u64 r0, u64 n);
MI_LOCAL void zh_recode_encode_enqueue(mi_ctx* c, const u64* u_src, const u64* u_word, const u64* r_off, const u32* r_rule, u64 r0, u64 n,
                                       u64 base_off, void* scratch, void* scratch2, u32* r_cand, u32 waves);
MI_LOCAL void zh_rep_rows_enqueue(mi_ctx* c, const u64* rep, u64 n, const u64* r_word, const u32* r_new, const u64* r_addr, u64* v_src,
                                  u64* v_word);
MI_LOCAL void zh_redecode_enqueue(mi_ctx* c, const u64* rep, u64 n, const u64* v_src, const u64* v_word, const u64* r_off, u64 base_off,
                                  void* scratch, u64* v_off, u64* v_len, u64* n_bad, u64* first_bad, u32 waves);
// ... and behind the placing pass: e_src[k] = d_hsrc[k] where that is set
MI_LOCAL void zh_sources_enqueue(mi_ctx* c, const u64* d_hsrc, u64* e_src, u64 n);

}  // namespace mi
