// What gpry_leave_out (loo.hip) and gpry_predict_without (predict_without.hip) share: the description of a group of
// training points, the host checks of a list of groups and the launch of the two group kernels of loo.hip, which form
// B = (K^-1)_GG, its Cholesky factor, W = L_B^-1 and W alpha_G.  One code, hence the same bits in both calls.
#pragma once
#include "common.h"

#define LGO_MAX 64          // largest group
#define LGO_KC 256          // training rows per workgroup of the Gram
#define LGO_KS 32           // ... and per LDS step
#define LGO_LD 66           // row stride of the LDS images of the group kernels (chol_panel.hip's)
#define LGO_MAX_GROUPS (1 << 20)
#define LGO_BATCH_DOUBLES (int64_t(1) << 25)     // partial Grams of one batch of groups (256 MB)

struct LgoGroup {
    int64_t idx_off;        // first entry in the sorted index list (and in the per-index outputs)
    int64_t part_off;       // first double of the group's partial Grams: (nch - c0) slices of np x np
    int64_t cov_off;        // first double of its n x n covariance block
    int n, np, c0, pad;     // size, padded size, first chunk that holds a non-zero row
};

int lgo_parse_groups(gpry_ctx* ctx, const char* who, const int64_t* idx, const int64_t* offsets, int64_t ngroups,
                     std::vector<LgoGroup>* groups, std::vector<int>* sidx, std::vector<int>* perm, int64_t* ncov);
void lgo_launch(gpry_ctx* ctx, const int* didx, const LgoGroup* dgroups, int64_t ng, double* dpart, double* omean, double* ocov,
                double* ochi2, double* ologpdf, int* oinfo, double* oW, double* oz);
