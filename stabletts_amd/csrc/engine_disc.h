// What the period and the resolution discriminator share (engine_period_disc.cpp, engine_resolution_disc.cpp): weight-normed convs
// whose effective weights w = v g / ||v|| are engine-owned, recomputed by st_finalize (new tensors) and by st_repack (an in-place
// update, on the caller's stream), and the entry sequences of st_*_disc_forward, _train_forward and _train_backward.  A kind
// supplies a DiscKind: its geometry check and its forward; its files keep the activation layout and the launch sequences.
// Not part of the C ABI.
#pragma once
#include "engine_internal.h"
#include "period_disc_launch.h"

#include <algorithm>
#include <map>
#include <string>

namespace sthost {

constexpr const char* kWnG = "parametrizations.weight.original0";
constexpr const char* kWnV = "parametrizations.weight.original1";
struct WnConv { std::string name; float* w; int cout; int64_t numel; };      // parameter-name prefix, effective weight, its shape

struct DiscState : HeldState {
    std::vector<WnConv> convs;
    // the weight norm of every conv, as kernels on `s`; drops the held activations
    int weights(st_engine* e, hipStream_t s) {
        for (const WnConv& c : convs)
            HIPCHK(e, st::launch_pd_weight_norm(P(e, c.name + kWnV), P(e, c.name + kWnG), c.w, c.cout, (int)(c.numel / c.cout), s));
        held.have = false;      // the held activations are of the weights before
        return ST_OK;
    }
    int finalize(st_engine* e) override {
        if (int rc = weights(e, nullptr)) return rc;
        HIPCHK(e, hipDeviceSynchronize());
        return ST_OK;
    }
    int repack(st_engine* e, hipStream_t s) override {
        if (!e->finalized) return e->fail(ST_ERR_STATE, "st_repack after st_bind_param / st_load_param of a new pointer: call st_finalize");
        HIPCHK(e, hipSetDevice(e->device));
        return weights(e, s);
    }
};

// Geom: what the kind's check derives from (B, T) for its launch sequences
template <class Geom> struct DiscKind {
    Kind kind;
    int n_maps;                     // feature maps a forward returns
    const char* train_entry;        // the entry-point family, as sd_train_check's messages name it
    int (*check)(st_engine* e, int B, int T, Geom* g);
    // keep = nullptr: nothing is kept; else the activations the backward reads go to keep's buffer as well
    int (*forward)(st_engine* e, const float* x, float* const* fmaps, int B, const Geom& g, SdTrain* keep, hipStream_t s);
};

// st_*_disc_forward (train = false) and st_*_disc_train_forward
template <class Geom>
int disc_forward(const DiscKind<Geom>& k, st_engine* e, const float* x, float* const* fmaps, int B, int T, bool train, void* stream) {
    int rc = check_handle(e, k.kind); if (rc) return rc;
    if ((rc = check_finalized(e))) return rc;
    if (!x || !fmaps) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    for (int i = 0; i < k.n_maps; ++i) if (!fmaps[i]) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    Geom g;
    if ((rc = k.check(e, B, T, &g))) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    if (!train) return k.forward(e, x, fmaps, B, g, nullptr, (hipStream_t)stream);
    SdTrain* st = state_of<DiscState>(e)->begin();
    if ((rc = k.forward(e, x, fmaps, B, g, st, (hipStream_t)stream))) return rc;
    sd_train_commit(st, B, T, 0.0f, 0, false);
    return ST_OK;
}

// What disc_backward_begin hands a kind's backward launch sequence
struct DiscBackward {
    SdTrain* st = nullptr;          // the held forward; nullptr: neither gradient is wanted, nothing to launch
    hipStream_t s = nullptr;
    size_t wmax = 0;                // floats of the largest effective weight (0 without grad_flat): the size of dW
    float* dW = nullptr;            // set by the kind once its scratch is laid out: the weight-shaped plane wn_bwd reads
    float* grad_flat = nullptr;
    std::map<std::string, int64_t> goff;      // the gradient-offset table (train_grad_layout)
    float* G(const std::string& n) const { return grad_flat + goff.at(n); }
    // d w (in dW) -> d g, d v of convs[k]
    hipError_t wn_bwd(st_engine* e, int k) const {
        const WnConv& c = state_of<DiscState>(e)->convs[k];
        return st::launch_pd_weight_norm_bwd(dW, P(e, c.name + kWnV), P(e, c.name + kWnG), G(c.name + kWnV), G(c.name + kWnG), c.cout,
                                             (int)(c.numel / c.cout), s);
    }
};

// The prologue of st_*_disc_train_backward: the checks, the held forward, the device
template <class Geom>
int disc_backward_begin(const DiscKind<Geom>& k, st_engine* e, const float* const* d_fmaps, float* d_x, float* grad_flat, int B, int T, void* stream,
                        Geom* g, DiscBackward* bw) {
    int rc = check_handle(e, k.kind); if (rc) return rc;
    if (!d_fmaps) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if ((rc = k.check(e, B, T, g))) return rc;
    DiscState* ds = state_of<DiscState>(e);
    if ((rc = sd_train_check(e, ds->held, k.train_entry, "T", -1, B, T))) return rc;
    if (!d_x && !grad_flat) return ST_OK;
    HIPCHK(e, hipSetDevice(e->device));
    bw->st = &ds->held; bw->s = (hipStream_t)stream; bw->grad_flat = grad_flat;
    if (grad_flat) for (const WnConv& c : ds->convs) bw->wmax = std::max(bw->wmax, (size_t)c.numel);
    train_grad_layout(e, &bw->goff);
    return ST_OK;
}

}  // namespace sthost
