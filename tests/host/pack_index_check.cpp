// Host-side check of the weight-layout index maps of stabletts_amd/csrc/common.h (compiled by tests/test_pack_index.py with
// hipcc --cuda-host-only; no GPU): ffn_stream_index (both stages) and qkv_frag_index must be bijections onto
// their buffers, and every source element must be hit exactly once; ffn_wino_index likewise (three planes per tap triple).
// The packing jobs (PackJob: pack_job_elems / pack_job_map / pack_job_find, what the pack kernels and the recorder run) are checked
// against nested-loop statements of the weight and the transposed layouts, and the list kernel's block search against the ranges
// the recorder assigns.
#include <cstdio>
#include <map>
#include <vector>
#include "../../stabletts_amd/csrc/common.h"

// Walks job j through pack_job_map: every offset of `want` (destination -> source, kPackZero = zero fill) is hit exactly once with
// that source, nothing else is, nothing lies at or beyond dst_size, and the element count is the number of pairs.
static int check_job(const st::PackJob& j, const std::map<size_t, size_t>& want, size_t dst_size, std::vector<int>* hits) {
    int bad = st::pack_job_elems(j) != want.size();
    for (size_t idx = 0; idx < st::pack_job_elems(j); ++idx) {
        const st::PackElem m = st::pack_job_map(j, idx);
        const auto it = want.find(m.dst);
        if (m.dst >= dst_size || it == want.end() || it->second != m.src || m.variant != 0) { ++bad; continue; }
        ++(*hits)[m.dst];
    }
    for (const auto& kv : want) bad += (*hits)[kv.first] != 1;
    return bad;
}

static int check_pack_jobs() {
    int bad = 0;
    std::vector<st::PackJob> list;
    float* const src = nullptr;
    {   // weight job: (3, 7, 3) source, channels [2, 6) into columns [8, 14) of rows 2.. of a [.][3][16] buffer, two columns of zeros
        const int cout = 3, cin_total = 7, K = 3, ci_off = 2, ci_cnt = 4, row_off = 2, cin_p = 16, col_off = 8, slice_w = 6;
        std::map<size_t, size_t> want;
        for (int co = 0; co < cout; ++co)
            for (int t = 0; t < K; ++t)
                for (int ci = 0; ci < slice_w; ++ci)
                    want[(size_t)((row_off + co) * K + t) * cin_p + col_off + ci] = ci < ci_cnt ? (size_t)((co * cin_total + ci_off + ci) * K + t) : st::kPackZero;
        const size_t n = (size_t)(row_off + cout) * K * cin_p;
        std::vector<int> hits(n, 0);
        const st::PackJob j = st::pack_job_weight(src, cout, cin_total, K, ci_off, ci_cnt, nullptr, row_off, cin_p, col_off, slice_w, 0);
        bad += check_job(j, want, n, &hits);
        size_t total = 0;
        for (int h : hits) total += h;
        bad += total != (size_t)cout * K * slice_w;      // nothing outside the slice was touched
        list.push_back(j);
    }
    {   // split triple [W_hi | W_hi | W_lo]: three column slices fill [2][1][24] exactly once
        const int cout = 2, cin = 8, cin_p = 24;
        std::vector<int> hits((size_t)cout * cin_p, 0);
        for (int part = 0; part < 3; ++part) {
            std::map<size_t, size_t> want;
            for (int co = 0; co < cout; ++co)
                for (int ci = 0; ci < cin; ++ci) want[(size_t)co * cin_p + part * cin + ci] = (size_t)co * cin + ci;
            const st::PackJob j = st::pack_job_weight(src, cout, cin, 1, 0, cin, nullptr, 0, cin_p, part * cin, cin, part == 2);
            bad += j.lo != (part == 2);
            bad += check_job(j, want, hits.size(), &hits);
            list.push_back(j);
        }
        for (int h : hits) bad += h != 1;
    }
    {   // transposed (dgrad) job: Wd[ci][t][col_off + co] = W[co][ci_off + ci][taps - 1 - t]
        const int cout = 5, cin_total = 7, taps = 3, ci_off = 2, ci_cnt = 4, ld = 8, col_off = 2;
        std::map<size_t, size_t> want;
        for (int ci = 0; ci < ci_cnt; ++ci)
            for (int t = 0; t < taps; ++t)
                for (int co = 0; co < cout; ++co)
                    want[(size_t)(ci * taps + t) * ld + col_off + co] = (size_t)((co * cin_total + ci_off + ci) * taps + (taps - 1 - t));
        std::vector<int> hits((size_t)ci_cnt * taps * ld, 0);
        const st::PackJob j = st::pack_job_weight_t(src, cout, cin_total, taps, ci_off, ci_cnt, nullptr, ld, col_off);
        bad += st::pack_job_elems(j) != 60;
        bad += check_job(j, want, hits.size(), &hits);
        list.push_back(j);
    }
    {   // fp32 copy of 300 floats: the identity, two blocks
        const st::PackJob j = st::pack_job_copy(nullptr, src, 300);
        bad += st::pack_job_elems(j) != 300 || st::pack_job_blocks(j) != 2;
        for (size_t idx = 0; idx < 300; ++idx) { const st::PackElem m = st::pack_job_map(j, idx); bad += m.src != idx || m.dst != idx; }
        list.push_back(j);
    }
    // block ranges as the recorder assigns them: blk0 = running sum of ceil(elems / 256); the list kernel's search finds, for
    // every block of the merged grid, the job whose range holds it
    unsigned nblocks = 0;
    size_t by_elems = 0;
    for (st::PackJob& j : list) { j.blk0 = nblocks; nblocks += st::pack_job_blocks(j); by_elems += (st::pack_job_elems(j) + 255) / 256; }
    bad += nblocks != by_elems || list.size() != 6;
    for (unsigned b = 0; b < nblocks; ++b) {
        const int k = st::pack_job_find(list.data(), (int)list.size(), b);
        bad += k < 0 || k >= (int)list.size() || b < list[k].blk0 || b >= list[k].blk0 + st::pack_job_blocks(list[k]);
    }
    return bad;
}

int main() {
    int bad = check_pack_jobs();
    for (int F : {256, 512, 1024, 2048})
        {
            const size_t n = (size_t)F * 256 * 3;
            std::vector<unsigned char> dst(2 * n, 0);
            for (int stage = 0; stage < 2; ++stage) {
                std::vector<unsigned char> src(n, 0);
                for (size_t idx = 0; idx < n; ++idx) {
                    size_t so, dof;
                    st::ffn_stream_index(idx, stage, F, &so, &dof);
                    if (so >= n || dof >= 2 * n) { ++bad; continue; }
                    ++src[so]; ++dst[dof];
                }
                for (size_t i = 0; i < n; ++i) bad += src[i] != 1;
            }
            for (size_t i = 0; i < 2 * n; ++i) bad += dst[i] != 1;
        }
    {
        std::vector<unsigned char> dst(3 * 256 * 256, 0);
        for (int plane = 0; plane < 3; ++plane)
            for (int co = 0; co < 256; ++co)
                for (int ci = 0; ci < 256; ++ci) {
                    const size_t d = st::qkv_frag_index(plane, co, ci);
                    if (d >= dst.size()) { ++bad; continue; }
                    ++dst[d];
                    // a wave's fragment (plane, co / 32, ci / 16) is one contiguous KiB, lane-linear
                    const size_t frag = d >> 9, lane = (d >> 3) & 63, e = d & 7;
                    bad += frag != (size_t)((plane * 8 + co / 32) * 16 + ci / 16) || lane != (size_t)(((ci >> 3) & 1) * 32 + (co & 31)) || e != (size_t)(ci & 7);
                }
        for (unsigned char c : dst) bad += c != 1;
    }
    // ffn_wino_index (the Winograd fused FFN's stream): per stage every (row, input channel) tap triple is used for exactly the three
    // planes, the two stages fill the stream exactly once, a wave's three fragments of a k-step are consecutive KiB, lane-linear
    for (int F : {256, 512, 1024, 2048}) {
        const size_t n = (size_t)F * 256 * 3;
        std::vector<unsigned char> dst(2 * n, 0);
        for (int stage = 0; stage < 2; ++stage) {
            std::vector<unsigned char> planes(n / 3, 0);
            for (size_t idx = 0; idx < n; ++idx) {
                size_t so, dof; int pl;
                st::ffn_wino_index(idx, stage, F, &so, &dof, &pl);
                if (so % 3 || so + 2 >= n || dof >= 2 * n || pl < 0 || pl > 2) { ++bad; continue; }
                planes[so / 3] |= (unsigned char)(1 << pl); ++dst[dof];
                const size_t frag = dof >> 9;                       // = (((chunk * 2 + stage) * 16 + k-step) * 8 + wave) * 3 + plane
                bad += (int)(frag % 3) != pl || (int)((frag / 3 / 8 / 16) & 1) != stage;
            }
            for (unsigned char c : planes) bad += c != 7;
        }
        for (unsigned char c : dst) bad += c != 1;
        const float g3[3] = {1.0f, 2.0f, 4.0f};
        bad += st::ffn_wino_plane(g3, 0) != 1.0f || st::ffn_wino_plane(g3, 1) != 3.5f || st::ffn_wino_plane(g3, 2) != 4.0f;
    }
    printf("bad %d\n", bad);
    return bad != 0;
}
