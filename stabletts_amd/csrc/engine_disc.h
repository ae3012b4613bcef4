// What the period and the resolution discriminator share (engine_period_disc.cpp, engine_resolution_disc.cpp): weight-normed convs
// whose effective weights w = v g / ||v|| are engine-owned, recomputed by st_finalize (new tensors) and by st_repack (an in-place
// update, on the caller's stream).  Not part of the C ABI.
#pragma once
#include "engine_internal.h"
#include "period_disc_launch.h"

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

}  // namespace sthost
