// C entry point for tests/test_head_fold_host.py: the host-side head fold of pf_host_prep.h, built with g++ alone.
#include "../../phyloformer_amd/csrc/pf_host_prep.h"

extern "C" void shim_fold_head(const float* w2, const float* b2, const float* hw, float hb, double w2_scale, float* u_img,
                               float* c0) {
    pfhost::fold_head(w2, b2, hw, hb, w2_scale, u_img, c0);
}
