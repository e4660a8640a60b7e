// dw_sensors.hip -- the kernel of the foot force-torque sensors (include/dyros_sensors.h).  The per-env arithmetic is
// dw_sensors.h's (the chain: dw_bodies.h's), shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
//   dwf_k_refresh  one launch.  61 words are read and at most 8 * 6 + 8 + 4 + 48 = 108 written per env: latency binds, not a stream.  A
//                  workgroup of 256 lanes takes DWF_GROUP = 16 envs.  The model table, the envs' root rows (one contiguous block), their 24 leg
//                  joint words and their impulse blocks (96 bytes out of a 1488-byte record, six 16-byte pieces each) come into LDS with
//                  consecutive lanes on consecutive words.  A lane per (env, foot), 32 lanes of the first wave, walks the foot's six links
//                  and leaves o_f = x_f - x_0 and R_f in LDS; the other three waves skip the phase.  A lane per output row (env, sensor | sole |
//                  zmp | corner), rows of one kind side by side, then forms its 4 or 6 words once into an LDS image of the group's output blocks, and consecutive lanes
//                  copy every block out, 16 bytes per lane where the output is 16-byte aligned (a group's block then is too).
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/dyros_walk.h"
#include "dw_group.h"
#include "dw_sensors.h"

namespace {

grp::Err s_err;
int fail(const char *msg) { return s_err.fail("dwf_refresh", msg); }

constexpr int G = dwf::G, TPB = 256;
static_assert(TPB % 64 == 0 && G * DWF_NUM_FEET <= 64, "whole waves; the chain lanes sit in one wave");
static_assert(DWF_ES_WARM % 4 == 0 && DWF_ES_WORDS % 4 == 0 && DWF_WARM_WORDS % 4 == 0, "16-byte pieces");
static_assert((G * DWF_SENSOR_WORDS) % 4 == 0 && (G * dwf::W_COP) % 4 == 0 && (G * dwf::W_ZMP) % 4 == 0 && (G * dwf::W_COR) % 4 == 0,
              "a group's output blocks start on 16 bytes");
static_assert(DWF_ES_WORDS == DW_ES_WORDS && DWF_ES_WARM == DW_ES_WARM && DWF_NUM_CORNERS == DW_NUM_FOOT_PTS && DWF_DOF_ROW == 2 * DW_NUM_DOF,
              "the task record's layout is dyros_walk.h's");
constexpr int OUT_WORDS = G * (dwf::NS * dwf::W_SEN + dwf::W_COP + dwf::W_ZMP + dwf::W_COR);
static_assert((DWB_TABLE_WORDS + G * (dwf::IN_ROOT + dwf::IN_DOF + dwf::IN_WARM + DWF_NUM_FEET * dwf::FP) + OUT_WORDS) * 4 <= 64 * 1024, "static LDS");

struct Sensors {
    DwfSensor s[DWF_MAX_SENSORS];
};

// n words of the LDS image to dst, consecutive lanes on consecutive words
__device__ inline void copy_out(float *__restrict__ dst, const float *src, int n, int t) {
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0u) {
        const int nv = n / 4;
        for (int i = t; i < nv; i += TPB) reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(src)[i];
        done = 4 * nv;
    }
    for (int i = done + t; i < n; i += TPB) dst[i] = src[i];
}

__global__ __launch_bounds__(TPB) void dwf_k_refresh(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                     const float *__restrict__ dof_state, const uint4 *__restrict__ env_state, DwfModel M,
                                                     Sensors sen, int ns, float *__restrict__ sensors, float *__restrict__ cop,
                                                     float *__restrict__ zmp, float *__restrict__ corners) {
    __shared__ uint4 s_tab4[DWB_TABLE_WORDS / 4];
    __shared__ float s_root[G * dwf::IN_ROOT];
    __shared__ float s_dof[G * dwf::IN_DOF];
    __shared__ uint4 s_warm4[G * dwf::IN_WARM / 4];
    __shared__ float s_fp[G * DWF_NUM_FEET * dwf::FP];
    __shared__ __attribute__((aligned(16))) float s_sen[G * dwf::NS * dwf::W_SEN];
    __shared__ __attribute__((aligned(16))) float s_cop[G * dwf::W_COP];
    __shared__ __attribute__((aligned(16))) float s_zmp[G * dwf::W_ZMP];
    __shared__ __attribute__((aligned(16))) float s_cor[G * dwf::W_COR];
    const int t = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = n - e0 < G ? n - e0 : G;          // envs of this workgroup (the last one may hold fewer)
    // ---- loads: consecutive lanes, consecutive words ----
    grp::load_table<TPB, DWB_TABLE_WORDS>(table, t, s_tab4);
    grp::load_rows<TPB>(root_states, e0, ne, dwf::IN_ROOT, t, s_root);
    {
        const float *src = dof_state + (size_t)e0 * DWF_DOF_ROW;
        for (int i = t; i < ne * dwf::IN_DOF; i += TPB) {
            const int e = i / dwf::IN_DOF;
            s_dof[i] = src[e * DWF_DOF_ROW + (i - e * dwf::IN_DOF)];
        }
        constexpr int PW = dwf::IN_WARM / 4;          // 16-byte pieces of an impulse block
        const uint4 *es = env_state + (size_t)e0 * (DWF_ES_WORDS / 4) + DWF_ES_WARM / 4;
        for (int i = t; i < ne * PW; i += TPB) {
            const int e = i / PW;
            s_warm4[i] = es[e * (DWF_ES_WORDS / 4) + (i - e * PW)];
        }
    }
    __syncthreads();
    const dwb::Tab T{reinterpret_cast<const uint32_t *>(s_tab4)};
    const float *s_warm = reinterpret_cast<const float *>(s_warm4);
    // ---- a lane per (env, foot): 32 lanes of one wave walk the six links of a leg ----
    if (t < ne * DWF_NUM_FEET) {
        const int e = t / DWF_NUM_FEET, f = t - DWF_NUM_FEET * e;
        dwf::foot_pose(T, f == 0 ? M.foot_mv[0] : M.foot_mv[1], s_root + e * dwf::IN_ROOT, s_dof + e * dwf::IN_DOF, s_fp + t * dwf::FP);
    }
    __syncthreads();
    // ---- a lane per output row, every row formed once; rows of one kind sit side by side (kind-major), so that a wave forms one kind ----
    const int rows_env = ns + DWF_NUM_FEET + 1 + dwf::NC;
    for (int i = t; i < ne * rows_env; i += TPB) {
        int r = i / ne;
        const int e = i - r * ne;
        const float *fps = s_fp + e * DWF_NUM_FEET * dwf::FP, *warm = s_warm + e * dwf::IN_WARM, *root = s_root + e * dwf::IN_ROOT;
        if (r < ns) {
            if (sensors != nullptr) dwf::sensor_row(M, sen.s[r], fps, warm, s_sen + (e * ns + r) * dwf::W_SEN);
        } else if ((r -= ns) < DWF_NUM_FEET) {
            if (cop != nullptr) dwf::cop_row(M, r, warm, s_cop + e * dwf::W_COP + r * DWF_COP_WORDS);
        } else if ((r -= DWF_NUM_FEET) < 1) {
            if (zmp != nullptr) dwf::zmp_row(M, fps, warm, root, s_zmp + e * dwf::W_ZMP);
        } else {
            r -= 1;
            if (corners != nullptr) dwf::corner_row(M, r, fps, warm, root, s_cor + e * dwf::W_COR + r * DWF_CORNER_WORDS);
        }
    }
    __syncthreads();
    // ---- the group's blocks, each contiguous ----
    if (sensors != nullptr) copy_out(sensors + (size_t)e0 * ns * dwf::W_SEN, s_sen, ne * ns * dwf::W_SEN, t);
    if (cop != nullptr) copy_out(cop + (size_t)e0 * dwf::W_COP, s_cop, ne * dwf::W_COP, t);
    if (zmp != nullptr) copy_out(zmp + (size_t)e0 * dwf::W_ZMP, s_zmp, ne * dwf::W_ZMP, t);
    if (corners != nullptr) copy_out(corners + (size_t)e0 * dwf::W_COR, s_cor, ne * dwf::W_COR, t);
}

}  // namespace

extern "C" {

int dwf_abi_version(void) { return DWF_ABI_VERSION; }
const char *dwf_last_error(void) { return s_err.s; }

int dwf_refresh(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *env_state,
                const DwfModel *model_host, const DwfSensor *sensors_host, int32_t ns, float *sensors, float *cop, float *zmp,
                float *corners, void *stream) {
    if (num_envs < 1 || num_envs > 0x7fffffff / DWF_ES_WORDS - G) return fail("num_envs must be in [1, 2^31 / 372 - 16)");
    if (!table || !root_states || !dof_state || !env_state) return fail("a buffer is missing");
    const char *why = dwf::refusal(model_host, sensors_host, ns);
    if (why) return fail(why);
    if ((ns > 0) != (sensors != nullptr)) return fail("sensors [N, ns, 6] must be given exactly when ns > 0");
    if (!sensors && !cop && !zmp && !corners) return fail("sensors, cop, zmp or corners must be given");
    if ((reinterpret_cast<uintptr_t>(table) & 15u) != 0u) return fail("the table must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(env_state) & 15u) != 0u) return fail("env_state must be 16-byte aligned");
    Sensors sen;
    memset(&sen, 0, sizeof(sen));
    for (int s = 0; s < ns; ++s) sen.s[s] = sensors_host[s];
    hipLaunchKernelGGL(dwf_k_refresh, dim3(dwf::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs,
                       reinterpret_cast<const uint4 *>(table), root_states, dof_state, reinterpret_cast<const uint4 *>(env_state), *model_host, sen,
                       (int)ns, sensors, cop, zmp, corners);
    return s_err.launched("dwf_refresh");
}

}  // extern "C"
