// CPU check of the vocoders' chunk planner (csrc/chunk_plan.h) against the two loops it replaced, restated here as they stood in
// st_vocos_forward_ragged and st_ffgan_forward_ragged (the caps as parameters, so that small ones make several chunks out of tens of
// utterances; FireflyGAN's 65535 items is max_items).  Per case: the starts are equal element for element, the chunks cover
// 0 .. B without gaps, and no chunk breaks a cap -- except one utterance alone above the head budget, which runs as before.
#include "../../stabletts_amd/csrc/chunk_plan.h"

#include <cstdio>
#include <random>

using sthost::ChunkLimits;

static std::vector<int> vocos_reference(const int64_t* lengths, int B, int T, int64_t max_rows, int64_t kVocMaxPaddedFrames) {
    std::vector<int> starts;          // first utterance of every chunk, then B
    int64_t rows = 0;
    for (int b = 0; b < B; ++b) {
        if (b == 0 || rows + lengths[b] > max_rows || (int64_t)(b - starts.back() + 1) * T > kVocMaxPaddedFrames) { starts.push_back(b); rows = 0; }
        rows += lengths[b];
    }
    starts.push_back(B);
    return starts;
}

static std::vector<int> ffgan_reference(const int64_t* lengths, int B, int64_t max_rows, int64_t head_rows, int64_t max_items) {
    std::vector<int> starts;          // first utterance of every chunk, then B
    int64_t rows = 0;
    for (int b = 0; b < B; ++b) {
        if (b == 0 || rows + lengths[b] > head_rows || rows + lengths[b] > max_rows || b - starts.back() >= max_items) { starts.push_back(b); rows = 0; }
        rows += lengths[b];
    }
    starts.push_back(B);
    return starts;
}

static int bad = 0, cases = 0;

static void fail(const char* what, const char* why, const std::vector<int64_t>& len, const std::vector<int>& got) {
    ++bad;
    printf("FAIL %s: %s; lengths", what, why);
    for (int64_t l : len) printf(" %lld", (long long)l);
    printf("; starts");
    for (int s : got) printf(" %d", s);
    printf("\n");
}

// `expect`: the starts worked out by hand for the named cases (empty: the reference alone)
static void check(const char* what, const std::vector<int64_t>& len, int T, const ChunkLimits& lim, const std::vector<int>& ref,
                  const std::vector<int>& expect = {}) {
    ++cases;
    const int B = (int)len.size();
    const std::vector<int> got = sthost::plan_chunks(len.data(), B, T, lim);
    if (got != ref) fail(what, "differs from the reference loop", len, got);
    if (!expect.empty() && got != expect) fail(what, "differs from the expected starts", len, got);
    if (got.size() < 2 || got.front() != 0 || got.back() != B) { fail(what, "does not cover 0 .. B", len, got); return; }
    for (size_t k = 0; k + 1 < got.size(); ++k) {
        const int b0 = got[k], b1 = got[k + 1];
        if (b1 <= b0) { fail(what, "empty or overlapping chunk", len, got); return; }
        int64_t rows = 0;
        for (int b = b0; b < b1; ++b) rows += len[b];
        const int64_t n = b1 - b0;
        if (rows > lim.max_rows) fail(what, "row cap broken", len, got);
        if (n > lim.max_items) fail(what, "item cap broken", len, got);
        if (lim.max_padded_frames && n * T > lim.max_padded_frames) fail(what, "padded-frame cap broken", len, got);
        if (lim.head_rows && rows > lim.head_rows && n != 1) fail(what, "head budget broken by more than one utterance", len, got);
    }
}

static const int64_t kNone = INT64_MAX;

static void vocos(const char* what, const std::vector<int64_t>& len, int T, int64_t max_rows, int64_t padded, const std::vector<int>& expect = {}) {
    check(what, len, T, ChunkLimits{max_rows, kNone, padded, 0}, vocos_reference(len.data(), (int)len.size(), T, max_rows, padded), expect);
}
static void ffgan(const char* what, const std::vector<int64_t>& len, int T, int64_t max_rows, int64_t head_rows, int64_t max_items,
                  const std::vector<int>& expect = {}) {
    check(what, len, T, ChunkLimits{max_rows, max_items, 0, head_rows}, ffgan_reference(len.data(), (int)len.size(), max_rows, head_rows, max_items), expect);
}

int main() {
    const int64_t big = 1 << 20;
    // all lengths equal: 30 utterances of 10 rows, 45 rows per chunk -> four a chunk
    vocos("vocos equal", std::vector<int64_t>(30, 10), 10, 45, big, {0, 4, 8, 12, 16, 20, 24, 28, 30});
    ffgan("ffgan equal", std::vector<int64_t>(30, 10), 10, 45, big, big, {0, 4, 8, 12, 16, 20, 24, 28, 30});
    ffgan("ffgan equal, head budget", std::vector<int64_t>(30, 10), 10, big, 45, big, {0, 4, 8, 12, 16, 20, 24, 28, 30});
    // one utterance exactly fills the row cap, and a chunk whose sum is exactly the cap
    vocos("vocos exact", {30, 100, 40, 60, 40, 1}, 100, 100, big, {0, 1, 2, 4, 6});
    ffgan("ffgan exact", {30, 100, 40, 60, 40, 1}, 100, 100, big, big, {0, 1, 2, 4, 6});
    ffgan("ffgan exact, head budget", {30, 100, 40, 60, 40, 1}, 100, big, 100, big, {0, 1, 2, 4, 6});
    // one row over the cap starts a new chunk
    vocos("vocos one over", {60, 41, 59, 1, 1}, 100, 100, big, {0, 1, 3, 5});
    ffgan("ffgan one over", {60, 41, 59, 1, 1}, 100, 100, big, big, {0, 1, 3, 5});
    // the item cap before the row cap
    ffgan("ffgan items", std::vector<int64_t>(11, 1), 8, 100, big, 4, {0, 4, 8, 11});
    // the padded-frame cap (count * T) before the row cap: T = 50, 120 padded frames -> two a chunk
    vocos("vocos padded", {3, 50, 1, 2, 7}, 50, 1000, 120, {0, 2, 4, 5});
    vocos("vocos padded, exactly", std::vector<int64_t>(7, 2), 40, 1000, 120, {0, 3, 6, 7});
    // one utterance alone above the head budget still runs, alone
    ffgan("ffgan above the head budget", {5, 80, 5, 5}, 80, 100, 20, big, {0, 1, 2, 4});
    ffgan("ffgan above the head budget, first", {80, 5}, 80, 100, 20, big, {0, 1, 2});
    // B = 1
    vocos("vocos B = 1", {17}, 40, 100, big, {0, 1});
    ffgan("ffgan B = 1", {17}, 40, 100, 50, 4, {0, 1});
    ffgan("ffgan B = 1 above the head budget", {17}, 40, 100, 3, 4, {0, 1});

    // pseudo-random length vectors, fixed seed: tens of utterances, caps small enough for several chunks
    std::mt19937 rng(20250607u);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    for (int it = 0; it < 400; ++it) {
        const int B = pick(1, 60), T = pick(1, 40);
        std::vector<int64_t> len(B);
        for (int64_t& l : len) l = pick(1, T);
        const int64_t max_rows = pick(T, 6 * T);                 // the entry points refuse a length above max_rows
        vocos("vocos random", len, T, max_rows, (int64_t)T * pick(1, 8) + pick(0, T - 1));      // ... and T above the padded-frame cap
        ffgan("ffgan random", len, T, max_rows, pick(1, 6 * T), pick(1, 9));
    }

    // the dense chunk size against the two expressions it replaced
    for (int B = 1; B <= 70; B += 3)
        for (int T = 1; T <= 40; T += 3)
            for (int64_t max_rows = T; max_rows <= 200; max_rows += 37)
                for (int64_t items : {(int64_t)1, (int64_t)5, (int64_t)65535}) {
                    ++cases;
                    const int vref = (int)std::min<int64_t>({(int64_t)B, max_rows / T, items});
                    if (sthost::dense_chunk(B, T, ChunkLimits{max_rows, items, 1 << 23, 0}) != vref) { ++bad; printf("FAIL dense vocos B %d T %d\n", B, T); }
                    for (int64_t kFfganHeadBytes : {(int64_t)1, (int64_t)1000, (int64_t)100000}) {
                        const int64_t per_row = 14 * 16;       // bytes of head workspace per row
                        const int64_t head_item = per_row * T, head_rows = std::max<int64_t>(1, kFfganHeadBytes / per_row);
                        const int fref = (int)std::min<int64_t>({(int64_t)B, std::max<int64_t>(1, kFfganHeadBytes / head_item), max_rows / T, items});
                        if (sthost::dense_chunk(B, T, ChunkLimits{max_rows, items, 0, head_rows}) != fref) { ++bad; printf("FAIL dense ffgan B %d T %d\n", B, T); }
                    }
                }
    printf("cases %d bad %d\n", cases, bad);
    return bad ? 1 : 0;
}
