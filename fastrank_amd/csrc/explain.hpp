// Interface between capi.cpp (which builds the tables from a model, explain_host.hpp) and explain.hip (which holds the
// kernels of the model explanation: the cover pass, TreeSHAP over the path table, the |phi| reduction).  DESIGN.md
// section 12 states the algorithm; tests/explain_model.py restates it in numpy, operation for operation.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace frdev {

constexpr uint32_t EX_MAX_PATH = 32;         // distinct features on one root-to-leaf path (elements of a path)
constexpr uint32_t EX_NO_FEATURE = 0xFFFFFFFFu;
constexpr size_t EX_LDS_MAX = 156 * 1024;    // bytes of LDS the explain kernel's one-wave workgroup may take
constexpr uint32_t EX_CHUNK_TILES = 1024;    // feature importance: 64-document tiles explained and reduced per launch

constexpr uint32_t EX_REG_PATH = 8;          // paths of up to this many elements keep their permutation weights in registers

// LDS of the explain kernel: the permutation weights [max_path + 1][64] f64 (none when no path is longer than EX_REG_PATH),
// a tree's accumulators [max_tree_feats][64] f64 and the documents' values of the tree's features [max_tree_feats][64] f32
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t ex_w_rows(uint32_t max_path) { return max_path > EX_REG_PATH ? max_path + 1 : 0; }
inline size_t ex_lds_bytes(uint32_t max_path, uint32_t max_tree_feats) {
    return (size_t)ex_w_rows(max_path) * 64 * 8 + (size_t)max_tree_feats * 64 * (8 + 4);
}

// The documents of one dataset handle, as the kernels visit them: document i sits at padded position pos[i] of the tiles
// and is instance ids[i] (positions ascending).
struct ExDocs {
    const float* xb = nullptr;
    uint32_t dq = 0, d = 0;
    int device = 0;
    std::vector<uint32_t> pos, ids;
};

// The trees as the cover pass walks them.  Node k: fid < 0 = a leaf, whose lhs holds its number over all trees (tree t's
// leaves are leaf0[t] .. leaf0[t + 1], depth first); else (double)x[fid] <= split goes to lhs, anything else to rhs.
struct ExWalk {
    std::vector<int32_t> fid, lhs, rhs, root;
    std::vector<double> split;
    std::vector<uint32_t> leaf0;  // [trees + 1]
};

// The path table.  Leaf L (numbered as above) has m[L] elements eoff[L] .. eoff[L] + m[L]; element e tests
// lo[e] < (double)x <= hi[e] on the tree's feature slot[e] and carries the background's cover ratio z[e].  Tree t's features
// are feat0[t] .. feat0[t + 1]: fid (EX_NO_FEATURE when the dataset does not hold it: it reads 0.0) and the output column col.
struct ExTables {
    std::vector<uint32_t> leaf0, feat0;     // [trees + 1]
    std::vector<double> weight;             // [trees]
    std::vector<uint32_t> m, eoff;          // [leaves]
    std::vector<double> value;              // [leaves]
    std::vector<uint32_t> slot;             // [elements]
    std::vector<double> lo, hi, z;          // [elements]
    std::vector<uint32_t> fid, col;         // [sum of the trees' features]
    uint32_t ncols = 0;                     // output columns: the features the model splits on
    uint32_t max_path = 0, max_tree_feats = 0;
};

struct ExTimes {
    double kernel_ms = 0.0, copy_ms = 0.0;
};

// counts[L] = documents of B that reach leaf L (integer atomics: the result does not depend on their order)
bool explain_covers(const ExDocs& B, const ExWalk& walk, std::vector<uint32_t>* counts, ExTimes* times, std::string* err);
// phi[i * ncols + c] for every document i of X (one launch; the device buffer is checked against `budget` bytes first)
bool explain_values(const ExDocs& X, const ExTables& tab, size_t budget, std::vector<double>* phi, ExTimes* times, std::string* err);
// sum_abs[c] = the sum over X's documents of |phi_c|, tile by tile in a fixed shape: a tile's 64 lanes in lane order, then
// the tiles in order; EX_CHUNK_TILES tiles are explained and reduced per launch, nothing larger is kept
bool explain_sum_abs(const ExDocs& X, const ExTables& tab, std::vector<double>* sum_abs, ExTimes* times, std::string* err);
// the (l, j) factors of EXTEND as the kernel reads them: fo[l * 33 + j] = (j + 1) / (l + 1), fz[l * 33 + j] = (l - j) / (l + 1)
void explain_factors(std::vector<double>* fo, std::vector<double>* fz);

}  // namespace frdev
