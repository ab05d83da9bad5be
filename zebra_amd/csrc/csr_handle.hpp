// The static adjacency's handle (zt_csr, include/zebra_amd.h): built and owned by tppr_prune.hip, read by seen.hip.
#pragma once
#include <vector>

#include "common.hpp"

struct zt_csr {
    int64_t N, E2;
    long long *indptr;  // device [N+1]
    int *nbr, *eid;     // device [2E]
    double *ts;         // device [2E]
    // host mirror (find_before on the host side of the shim, tests)
    std::vector<long long> h_indptr;
    std::vector<int> h_nbr, h_eid;
    std::vector<double> h_ts;
    // the workspace form's reservation (zt_csr_reserve_pruning); the query entry points take the handle const
    mutable void *ws = nullptr;              // device: ws_slabs x ws_slab_bytes
    long long ws_slab_bytes = 0;
    int ws_slabs = 0, ws_cap_c = 0, ws_cap_f = 0, ws_models = 0;
    hipEvent_t ws_event = nullptr;           // recorded after every workspace launch
    mutable hipStream_t ws_stream = nullptr; // the stream of the last one
    mutable bool ws_used = false;
};
