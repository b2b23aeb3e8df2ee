// A program of its own over csrc/forest_pack.hpp (the three encodings of a forest), for
// -fsanitize=address,undefined: forests at the packers' limits -- complete trees of 8 and 9 levels, chains of 10 and 11, 1023
// and 1024 thresholds on one feature, 170 and 171 features in use, a leaf-only tree, a feature id beyond d, a NaN split --
// packed by all three packers and by every block shape of the LDS walk.  It checks structure only (every index inside its
// buffer, the streams' padding, the descriptor lists' terminators); the values are tests/test_forest_pack_host.py's.
#include <cstdio>
#include <iterator>
#include <set>

#include "forest_pack.hpp"

using frdev::FlatTrees;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return false;                                               \
        }                                                               \
    } while (0)

static int32_t leaf(FlatTrees& t, double v) {
    t.fid.push_back(-1), t.lhs.push_back(-1), t.rhs.push_back(-1), t.split.push_back(v);
    return (int32_t)t.fid.size() - 1;
}
static int32_t split(FlatTrees& t, int32_t fid, double s, int32_t l, int32_t r) {
    t.fid.push_back(fid), t.lhs.push_back(l), t.rhs.push_back(r), t.split.push_back(s);
    return (int32_t)t.fid.size() - 1;
}
static int32_t complete(FlatTrees& t, uint32_t levels, uint32_t& count) {
    if (levels == 0) return leaf(t, 0.25 * (double)count++);
    const int32_t l = complete(t, levels - 1, count), r = complete(t, levels - 1, count);
    return split(t, (int32_t)(count % 24), 0.5 * (double)(count % 7) - 1.0, l, r);
}
static int32_t chain(FlatTrees& t, uint32_t depth) {
    int32_t n = leaf(t, 1.0);
    for (uint32_t k = depth; k-- > 0;) n = split(t, (int32_t)(k % 5), 0.125 * k, n, leaf(t, -(double)k));
    return n;
}
static void add_tree(FlatTrees& t, int32_t root, double w) { t.root.push_back(root), t.weight.push_back(w); }
static FlatTrees stumps(uint32_t count, bool one_feature) {
    FlatTrees t;
    for (uint32_t k = 0; k < count; k++)
        add_tree(t, split(t, one_feature ? 3 : (int32_t)k, one_feature ? 0.5 * k : 1.5, leaf(t, 1.0), leaf(t, 2.0)), 0.5 + k);
    return t;
}

static bool terminated(const std::vector<uint32_t>& desc, size_t end_units) {
    CHECK(desc.size() % 4 == 0 && desc.size() >= 8);
    const uint32_t* last = desc.data() + desc.size() - 4;
    CHECK(last[0] == end_units && last[1] == 0 && last[2] == 0 && last[3] == 0);
    return true;
}

static bool check_lds(const frdev::LdsForest& f, const frdev::TreeShape& sh, uint32_t d, uint32_t dq, size_t trees) {
    const size_t fixed = ((size_t)sh.docs * (dq * 4 + 1) * 4 + 15) / 16 * 16 + (sh.parts > 1 ? (size_t)sh.docs * 8 : 0);
    CHECK(f.lds_bytes <= 160 * 1024 && f.lds_bytes > fixed && f.forest.size() % 2 == 0);
    CHECK(terminated(f.desc, f.forest.size() / 2));
    CHECK(!f.leafprod.empty() && f.leafprod[0] == 0.0 && f.leafprod.size() <= (size_t(1) << 23));
    const uint32_t pad_off = dq * 4 * sh.docs * 4;
    size_t real = 0;
    for (size_t b = 0; b + 1 < f.desc.size() / 4; b++) {
        const size_t start = (size_t)f.desc[b * 4] * 2, end = (size_t)f.desc[b * 4 + 4] * 2, n = f.desc[b * 4 + 1];
        CHECK(start < end && end <= f.forest.size() && (end - start) * 8 <= f.lds_bytes - fixed);
        CHECK((n == 1 || n == 2 || n == 4 || n == 8 || n == 16) && n <= sh.nmax && sh.parts * n < end - start);
        CHECK((end - start) * 8 <= (size_t)sh.pf * 16 * sh.docs * sh.parts);  // what a prefetch slot of the block carries
        const uint64_t* w = f.forest.data() + start;
        const size_t len = end - start;
        std::vector<unsigned char> seen(len, 0);
        for (size_t i = 0; i < sh.parts * n; i++) {
            std::vector<std::pair<size_t, uint32_t>> work(1, {(size_t)(uint32_t)w[i], 0u});
            CHECK(w[i] >> 32 == 0);
            bool padding = true;
            while (!work.empty()) {
                const auto [at, depth] = work.back();
                work.pop_back();
                CHECK(at >= sh.parts * n && at < len && !seen[at]);
                seen[at] = 1;
                const uint32_t hi = (uint32_t)(w[at] >> 32), lo = (uint32_t)w[at], rel = hi >> 24, off = hi & 0xFFFFFF;
                CHECK(off % (sh.docs * 4) == 0 && (off / (sh.docs * 4) < d || off == pad_off));
                if (rel == 0) {  // a leaf: the 0.0 slot and a product index
                    CHECK(off == pad_off && lo < f.leafprod.size() && depth <= f.desc[b * 4 + 2]);
                    padding = padding && lo == 0 && depth == 0;
                } else {
                    work.push_back({at + rel, depth + 1}), work.push_back({at + rel + 1, depth + 1});
                }
            }
            real += padding ? 0 : 1;
        }
        for (size_t i = sh.parts * n; i < len; i++) CHECK(seen[i] || (i + 1 == len && w[i] == 0));  // one word of padding at most
    }
    CHECK(real == trees);
    return true;
}

static size_t leaves_of(const FlatTrees& t) {
    size_t leaves = 0;
    std::vector<int32_t> work(t.root.begin(), t.root.end());
    while (!work.empty()) {
        const int32_t at = work.back();
        work.pop_back();
        if (t.fid[at] < 0) leaves++;
        else work.push_back(t.lhs[at]), work.push_back(t.rhs[at]);
    }
    return leaves;
}

static bool check_rank(const frdev::RankForest& f, uint32_t d, uint32_t dq, size_t model_leaves) {
    constexpr uint32_t DOCS = frdev::RankBlock::DOCS, H = frdev::RankBlock::H, PF = frdev::RankBlock::PF;
    CHECK(f.fdesc.size() == (size_t)dq * 16 && f.rdesc.size() % (8 * H) == 0 && f.nrounds == f.rdesc.size() / (8 * H));
    std::set<uint32_t> slots;
    std::vector<uint32_t> tables_of(dq * 4, 0);
    for (uint32_t fi = 0; fi < dq * 4; fi++) {
        const uint32_t* fd = f.fdesc.data() + fi * 4;
        if (fd[0] == 0xFFFFFFFFu) continue;
        CHECK(fi < d && fd[0] + 2 <= 0xFFFF && fd[2] >= 1 && fd[2] <= 10 && fd[3] == 1u << fd[2] && slots.insert(fd[0]).second);
    }
    CHECK(slots.size() == f.nslots);
    const uint32_t p0 = (f.nslots >> 1) * DOCS * 4 + (f.nslots & 1) * 2, p1 = ((f.nslots + 1) >> 1) * DOCS * 4 + ((f.nslots + 1) & 1) * 2;
    CHECK(p1 <= 0xFFFF && !slots.count(p0) && !slots.count(p1));
    CHECK(f.lds_bytes == (((size_t)f.nslots + 3) / 2 * DOCS * 4 + 15) / 16 * 16 + (size_t)DOCS * 8 + (size_t)PF * 16 * DOCS * H && f.lds_bytes <= 160 * 1024);
    for (size_t r = 0; r < f.rdesc.size() / 8; r++) {
        const uint32_t* rd = f.rdesc.data() + r * 8;
        if (rd[2] == 0xFFFFFFFFu) continue;
        CHECK(rd[2] < dq && rd[2] % H == r % H && rd[1] % DOCS == 0 && rd[1] >= DOCS && rd[1] <= 8 * DOCS && (size_t)rd[0] + rd[1] <= f.tables.size());
        for (uint32_t j = 0; j < 4; j++) {
            if (rd[4 + j] == 0xFFFFFFFFu) continue;
            const uint32_t fi = rd[2] * 4 + ((rd[3] >> (8 + 2 * j)) & 3u);
            CHECK(f.fdesc[fi * 4] != 0xFFFFFFFFu && rd[4 + j] + f.fdesc[fi * 4 + 3] <= rd[1]);
            tables_of[fi]++;
        }
    }
    for (uint32_t fi = 0; fi < dq * 4; fi++) CHECK(tables_of[fi] == (f.fdesc[fi * 4] != 0xFFFFFFFFu ? 1u : 0u));
    CHECK(f.forest.size() % 4 == 0 && terminated(f.desc, f.forest.size() / 4));
    size_t leaves = 0;
    for (size_t b = 0; b + 1 < f.desc.size() / 4; b++) {
        const size_t start = (size_t)f.desc[b * 4] * 4, end = (size_t)f.desc[b * 4 + 4] * 4, n = f.desc[b * 4 + 1], L = f.desc[b * 4 + 2], leafbase = f.desc[b * 4 + 3];
        const size_t stride = (size_t(6) << L) / 4, next_base = b + 2 < f.desc.size() / 4 ? f.desc[b * 4 + 7] : f.leafprod.size();
        CHECK((n == 1 || n == 2 || n == 4 || n == 8) && L >= 1 && L <= 10 && start < end && end <= f.forest.size());
        CHECK(end - start == (H * n * stride + 3) / 4 * 4 && (end - start) * 4 <= (size_t)PF * 16 * DOCS * H);
        CHECK(leafbase < next_base && next_base <= f.leafprod.size() && next_base - leafbase <= 0x10000 && f.leafprod[leafbase] == 0.0);
        for (size_t i = 0; i < H * n; i++) {
            const uint32_t* nodes = f.forest.data() + start + i * stride;
            const uint16_t* ids = (const uint16_t*)(nodes + (size_t(1) << L));
            for (size_t h = 1; h < size_t(1) << L; h++) {
                const uint32_t off = nodes[h] & 0xFFFF, j = nodes[h] >> 16;
                CHECK(off == p0 || off == p1 || slots.count(off));
                CHECK(j < 1024 && ((off != p0 && off != p1) || j == 0));
            }
            for (size_t h = 0; h < size_t(1) << L; h++) CHECK(leafbase + ids[h] < next_base);
        }
        leaves += next_base - leafbase - 1;
    }
    CHECK(leaves == model_leaves);  // every batch's products: +0.0 for its padding trees, then one per leaf
    return true;
}

static bool check_l2(const FlatTrees& t) {
    std::vector<frdev::TreeNodeDev> nodes;
    std::vector<int32_t> roots;
    frdev::adjacent_children_layout(t, nodes, roots);
    CHECK(roots.size() == t.root.size());
    for (size_t k = 0; k < roots.size(); k++) {
        const size_t begin = (size_t)roots[k], end = k + 1 < roots.size() ? (size_t)roots[k + 1] : nodes.size();
        CHECK(begin < end && end <= nodes.size() && (end - begin) % 2 == 1);
        for (size_t i = begin; i < end; i++)
            CHECK(nodes[i].fid < 0 ? nodes[i].lhs == 0 : ((size_t)nodes[i].lhs > i && (size_t)nodes[i].lhs + 1 < end));
    }
    return true;
}

// packs `t` every way; returns false on a structural fault.  rank / lds: whether the rank encoding and any block shape took it
static bool pack_all(const char* what, const FlatTrees& t, uint32_t d, bool* rank, bool* lds) {
    const uint32_t dq = (d + 3) / 4;
    const frdev::ForestPackOptions opt;
    frdev::RankForest rf;
    *rank = frdev::pack_forest_rank(t, d, dq, opt, &rf);
    if (*rank) CHECK(check_rank(rf, d, dq, leaves_of(t)));
    *lds = false;
    frdev::LdsForest lf;  // one result record over every shape, as a caller that tries them in turn would keep it
    for (const frdev::TreeShape& sh : frdev::TREE_SHAPES) {
        if (t.raw_single && sh.parts != 1) continue;
        if (!frdev::pack_forest_lds(t, sh, d, dq, opt, &lf)) continue;
        *lds = true;
        CHECK(check_lds(lf, sh, d, dq, t.root.size()));
    }
    CHECK(check_l2(t));
    CHECK(frdev::forest_hash(t) != 0);
    std::printf("%-22s rank %d lds %d\n", what, (int)*rank, (int)*lds);
    return true;
}

static bool run() {
    bool rank = false, lds = false;
    uint32_t count = 0;
    for (uint32_t levels : {8u, 9u}) {
        FlatTrees t;
        add_tree(t, complete(t, levels, count), 0.5);
        add_tree(t, chain(t, 1), -2.0);
        CHECK(pack_all(levels == 8 ? "complete 8" : "complete 9", t, 24, &rank, &lds) && rank && lds == (levels == 8));
    }
    for (uint32_t depth : {10u, 11u}) {
        FlatTrees t;
        for (int k = 0; k < 5; k++) add_tree(t, chain(t, k == 2 ? depth : 2), 1.0 + k);
        CHECK(pack_all(depth == 10 ? "chain 10" : "chain 11", t, 24, &rank, &lds) && rank == (depth == 10) && lds);
    }
    for (uint32_t n : {1023u, 1024u}) {
        const FlatTrees t = stumps(n, true);
        CHECK(pack_all(n == 1023 ? "1023 thresholds" : "1024 thresholds", t, 24, &rank, &lds) && rank == (n == 1023) && lds);
    }
    for (uint32_t n : {170u, 171u}) {
        const FlatTrees t = stumps(n, false);
        CHECK(pack_all(n == 170 ? "170 features" : "171 features", t, 176, &rank, &lds) && rank == (n == 170) && lds);
    }
    {
        FlatTrees t;
        add_tree(t, leaf(t, -0.0), 3.0);
        CHECK(pack_all("one leaf", t, 24, &rank, &lds) && rank && lds);
        t.raw_single = true;
        CHECK(pack_all("one bare leaf", t, 24, &rank, &lds) && !rank && lds);
    }
    {
        FlatTrees t;  // features the dataset does not have, thresholds either side of the 0.0 they read, a NaN split
        add_tree(t, split(t, 24, -1.0, leaf(t, 1.0), split(t, 1000, 0.0, leaf(t, 2.0), leaf(t, 3.0))), 1.0);
        add_tree(t, split(t, 2, std::numeric_limits<double>::quiet_NaN(), leaf(t, 4.0), split(t, 23, -0.0, leaf(t, 5.0), leaf(t, 6.0))), 1.0);
        add_tree(t, split(t, 25, std::numeric_limits<double>::quiet_NaN(), leaf(t, 7.0), leaf(t, 8.0)), 1.0);
        CHECK(pack_all("absent and NaN", t, 24, &rank, &lds) && rank && lds);
        CHECK(pack_all("absent and NaN, d 1", t, 1, &rank, &lds) && rank && lds);
        t.weight[1] = std::nextafter(t.weight[1], 2.0);
        const uint64_t moved = frdev::forest_hash(t);
        t.weight[1] = 1.0;
        CHECK(moved != frdev::forest_hash(t));
    }
    {
        FlatTrees t;  // a bare chain: one-part blocks only
        t.raw_single = true;
        add_tree(t, chain(t, 40), 1.0);
        CHECK(pack_all("bare chain 40", t, 24, &rank, &lds) && !rank && lds);
    }
    {
        const FlatTrees none;
        frdev::RankForest rf;
        frdev::LdsForest lf;
        CHECK(!frdev::pack_forest_rank(none, 24, 6, frdev::ForestPackOptions(), &rf) && !frdev::pack_forest_lds(none, frdev::TREE_SHAPES[0], 24, 6, frdev::ForestPackOptions(), &lf));
        CHECK(check_l2(none) && frdev::tree_plan_batches({}).empty());
    }
    return true;
}

int main() {
    if (!run()) return 1;
    std::printf("forest_pack ok\n");
    return 0;
}
