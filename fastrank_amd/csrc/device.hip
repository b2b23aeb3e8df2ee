// HIP kernels + launchers for the fastrank hot path on MI355X (gfx950, wave64).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off  (contract=off is REQUIRED: the
// reference's dot product is an unfused f64 multiply-then-add, src/dense_dataset.rs:71-74).
//
// One translation unit, split into parts for reading:
//   device_plumbing.inc     HIP error macro, HIP-event kernel timing, device buffers
//   kernels_score.inc       tile layout (xb_index) + score_linear_kernel (exact ordered f64 dot
//                           product, lane = document), single-feature / axpy helpers
//   kernels_tree.inc        tree_ensemble_lds_kernel (forest streamed through LDS, 8 walks per lane)
//   kernels_treerank.inc    tree_ensemble_rank_kernel (threshold ranks instead of features: u16 codes, 32-bit heap nodes)
//                           and tree_ensemble_kernel (L2 fallback)
//   kernels_metric.inc      metric_sort_kernel (LDS bitonic sort + NDCG/AP/RR in the reference's
//                           summation order, and DCG / precision / recall / success / ERR) and the fixed-shape mean reduction
//   kernels_metric_topk.inc metric_topk_kernel: the five cut-off measures by selecting the first k ranks, one wave per
//                           (query, slot), no sort (measures_host.hpp: names, norms, definitions, the routing rule; host only)
//   kernels_linesearch.inc  linesearch_ndcg_kernel: the exact fused NDCG@k line search
//   kernels_verify.inc      linesearch_verify_kernel: bound-and-verify NDCG@k line search (the hot path; the exact
//                           kernel recomputes the pairs it cannot verify)
//   kernels_order.inc       xslot_kernel / rslot_kernel: the verify kernel's visiting-order tables (by x_f, by the resident sums)
//   kernels_fullrank.inc    linesearch_scores_kernel + rank_metric_kernel: AP / RR / depth-less NDCG
//   kernels_rr.inc          rr_verify_kernel / rr_exact_kernel: reciprocal rank by bound-and-verify
//   fullverify.hpp          interface to fullverify.hip (own objects, compiled per slice of the size classes):
//     kernels_sortnet.inc     (generated, tools/gen_sortnet.py) compare-exchange networks over register-resident keys
//     kernels_fullverify.inc  fullrank_verify_kernel: NDCG of any depth / AP by sorting approximate keys in registers
//                             and verifying the gaps (the exact kernels of kernels_fullrank.inc redo what fails)
//   kernels_rf.inc          random-forest TRAINING: level-synchronous split search over a batch of trees (rocPRIM radix sort +
//                           sequential-association importance kernels)
//   kernels_lambda.inc      lambda_grad_kernel: LambdaMART's LambdaRank gradients, one workgroup per query;
//                           lambda_grad_trunc_kernel: the same under a truncation level / per-query normalisation
//                           (both are templates over the objective: NDCG, MAP or MRR pair weights)
//   kernels_xendcg.inc      lambda_grad_xe_kernel: LambdaMART's listwise objective, one wave per query, O(n) per query
//   kernels_hist.inc        LambdaMART's histogram grower: one-byte bins, int64 fixed-point gradients, per-node histograms
//   kernels_histreg.inc     the histogram grower's scan kernels under lambda_l1 / max_delta_step / path_smooth
//   kernels_goss.inc        LambdaMART's gradient-based one-side sampling: an on-device radix select of the n-th largest |lambda|,
//                           the kept documents' list, amplified fixed-point gradients
//   kernels_histquant.inc   LambdaMART's quantised gradients: (q, w) of a few bits per entry under a per-tree key, and the histogram
//                           build over them with one packed 64-bit LDS atomic per update (arithmetic: lambdamart_quant.hpp)
//   kernels_dart.inc        LambdaMART's DART boosting: the u16 leaf cache and dart_rescore_kernel, which re-forms the scores
//                           of any weighting of the trees from it
//   dataset_layout.hpp      (through device.hpp; host only, no HIP) the layout arithmetic of a dataset: runs, size classes, gain
//                           tables, duplicate groups, walk tiles, a view's tables
//   linesearch_policy.hpp   (host only, no HIP) the adaptive policies of the bound-and-verify line search: routing / back-off of
//                           tie-heavy restarts, the R-rank refresh schedule, list length, redo grid, skip counter
//   forest_pack.hpp         (host only, no HIP) the three encodings of a forest the tree kernels read and their limits: the packers
//                           for tree_ensemble_rank_kernel and tree_ensemble_lds_kernel (block shapes, try-orders), the adjacent-children
//                           layout of the L2 walk and of permute_trees_kernel, the packed-forest cache's hash
//   device_dataset.inc      DeviceDataset: its state (Impl), the scoring and metric launchers, the whole line search; includes
//     dataset_build.inc       the uploads of that layout (tiles, tables): create, replicate, views
//     score_trees.inc         forest scoring: the launchers of kernels_treerank.inc and kernels_tree.inc over forest_pack.hpp's buffers,
//                             the packed-forest cache, the plan of the last call
//     train_rf.inc            the launchers of kernels_rf.inc
//     train_lambda.inc        the launchers of kernels_lambda.inc and kernels_xendcg.inc
//     train_dart.inc          the launchers of kernels_dart.inc
//     train_hist.inc          the launchers of kernels_hist.inc and kernels_histreg.inc, level-wise and leaf-wise, of kernels_goss.inc and kernels_histquant.inc
//   kernels_text.inc        the device text parser's kernels (line scan, the two parsing passes); text_parse.inc launches them
//                           (text_parse.hpp: the interface loader.hpp uses; text_number.hpp: grammar and value rule)
//   kernels_resample.inc    resample_boot_kernel / resample_perm_kernel: paired bootstrap and per-query permutation of a table of
//                           per-query values, a lane per trial; resample.inc launches them (resample.hpp: the interface and the
//                           definition; resample_host.hpp: the report the host makes of their output)
//   kernels_permute.inc     permute_linear_kernel / permute_trees_kernel / permute_single_kernel: a model's scores on the dataset
//                           with one column read from other rows, a chunk of columns and every repeat at once; permute.inc launches
//                           them (permute.hpp: the interface and the definition; permute_host.hpp: stream, options, report)
#include "device.hpp"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "forest_pack.hpp"
#include "fullverify.hpp"
#include "linesearch_policy.hpp"
#include "measures_host.hpp"
#include "verify_end.hpp"
#define FR_QUANT_ARITHMETIC_ONLY  // (lambdamart_quant.hpp without host.hpp: the integer arithmetic the kernels share with the host)
#include "lambdamart_quant.hpp"
#include "text_parse.hpp"
#include "resample.hpp"

#include <cstring>
#include <dlfcn.h>
#include <unistd.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <condition_variable>
#include <mutex>
#include <optional>
#include <thread>
#include <type_traits>

namespace frdev {

#include "device_plumbing.inc"
#include "kernels_score.inc"
#include "kernels_tree.inc"
#include "kernels_treerank.inc"
#include "kernels_metric.inc"
#include "kernels_metric_topk.inc"
#include "kernels_linesearch.inc"
#include "kernels_chain.inc"
#include "kernels_order.inc"
#include "kernels_verify.inc"
#include "kernels_fullrank.inc"
#include "kernels_rr.inc"
#include "kernels_rf.inc"
#include "kernels_lambda.inc"
#include "kernels_xendcg.inc"
#include "kernels_hist.inc"
#include "kernels_histreg.inc"
#include "kernels_goss.inc"
#include "kernels_histquant.inc"
#include "kernels_dart.inc"
#include "device_dataset.inc"
#include "rccl_exchange.inc"
#include "kernels_text.inc"
#include "text_parse.inc"
#include "kernels_resample.inc"
#include "resample.inc"
#include "kernels_permute.inc"
#include "permute.inc"

}  // namespace frdev
