// mmvae_encode's latent launch: the encode forms of the forward pass's latent kernel (lat_fwd.hpp, ENC 1 and 2), in a
// translation unit of their own so that rowwise.hip compiles the forward pass's forms exactly as it did without them.
#include "lat_fwd.hpp"

namespace mmvae {

int launch_lat_enc(const Ctx& c, const mmvae_noise* nz, const float* params, float* bn_running, int64_t* nbt,
                   const EncOut& eo, int32_t* labels_ab) {
    LatArgs a = make_lat_args(c);
    a.labels = labels_ab;
    NoiseDev nd = make_noise_dev(nz, c.h);
    const size_t shm = lat_smem_bytes(c.d);
    const dim3 grid(c.lay.nblkl, c.d.A);
    if (c.plan.lat_half) {
        auto k = eo.head ? k_lat_fwd_g<32, LH_NW, 2, EncOut> : k_lat_fwd_g<32, LH_NW, 1, EncOut>;
        hipLaunchKernelGGL(k, grid, dim3(64 * LH_NW), shm, c.stream, a, nd, params, c.ws, bn_running, nbt, eo);
    } else {
        auto k = eo.head ? k_lat_fwd_g<64, LAT_NW, 2, EncOut> : k_lat_fwd_g<64, LAT_NW, 1, EncOut>;
        hipLaunchKernelGGL(k, grid, dim3(64 * LAT_NW), shm, c.stream, a, nd, params, c.ws, bn_running, nbt, eo);
    }
    HIP_LAUNCH_CHECK("k_lat_enc");
    return 0;
}

}  // namespace mmvae
