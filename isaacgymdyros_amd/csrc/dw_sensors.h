// dw_sensors.h -- one env's foot force-torque sensors (include/dyros_sensors.h), written once for the HIP kernel of dw_sensors.hip and for a
// g++ build (tests/force_sensors_host.cpp), which the CPU tests hold against a float64 numpy restatement.  Two pieces: foot_pose (the
// chain from the base down to a foot, by dw_bodies.h's link arithmetic) and one function per output row (sensor_row, cop_row, zmp_row,
// corner_row), each from the env's two foot poses [2][FP] (offset from the base [3], rotation [9]), its 24 impulse words and its root row.
#ifndef DW_SENSORS_H
#define DW_SENSORS_H

#include "../../include/dyros_sensors.h"
#include "dw_bodies.h"

#define DWF_HD DWB_HD

namespace dwf {

constexpr int G = DWF_GROUP, NS = DWF_MAX_SENSORS, NC = DWF_NUM_CORNERS, CPF = DWF_NUM_CORNERS / DWF_NUM_FEET;
constexpr int IN_ROOT = 13, IN_DOF = 2 * DWF_LEG_DOF, IN_WARM = DWF_WARM_WORDS, FP = 12;
constexpr int W_SEN = DWF_SENSOR_WORDS, W_COP = DWF_NUM_FEET * DWF_COP_WORDS, W_ZMP = DWF_ZMP_WORDS, W_COR = NC * DWF_CORNER_WORDS;

DWF_HD int groups(int n) { return (n + G - 1) / G; }

// R^T v
DWF_HD void m3tv(const float *R, const float *v, float *o) {
    for (int i = 0; i < 3; ++i) o[i] = R[i] * v[0] + R[3 + i] * v[1] + R[6 + i] * v[2];
}

// the pose of moving body `body` (a leg body, 1..DWF_LEG_DOF) at root / dof (the env's first IN_DOF joint words): fp[0:3] = x_f - x_0,
// fp[3:12] = R_f.  The body is looked up in the table's root-to-leaf paths and the path walked down to it; a body that is on no path, or
// a path that leaves the legs, gives the pose reached so far (dwf_refresh and the Python layer refuse such a model; nothing is indexed
// past a store).
DWF_HD void foot_pose(const dwb::Tab &T, int body, const float *root, const float *dof, float *fp) {
    int l = 0, depth = 0;
    const int nleaf = T.nleaf();
    for (int p = 0; p < nleaf; ++p) {
        const int n = T.pathlen(p);
        for (int k = 0; k < n; ++k)
            if ((T.path(p, k) & 255) == body && depth == 0) { l = p; depth = k + 1; }
    }
    dwb::Body B;
    dwb::base(T, root, 0, B);
    for (int k = 0; k < depth; ++k) {
        const int b = T.path(l, k) & 255;
        if (b < 1 || b > DWF_LEG_DOF) break;
        dwb::child(T, b, dof, B);
    }
    for (int i = 0; i < 3; ++i) fp[i] = B.off[i];
    for (int i = 0; i < 9; ++i) fp[3 + i] = B.R[i];
}

// the force on corner k, world axes
DWF_HD void corner_force(const DwfModel &M, const float *warm, int k, float *f) {
    for (int i = 0; i < 3; ++i) f[i] = warm[3 * k + i] * M.inv_dt;
}

// sensor row [6]: fps = the env's [2][FP] foot poses, warm = its 24 impulse words
DWF_HD void sensor_row(const DwfModel &M, const DwfSensor &S, const float *fps, const float *warm, float *out) {
    const int f = S.foot == 1 ? 1 : 0;
    const float *R = fps + f * FP + 3;
    float F[3] = {0.0f, 0.0f, 0.0f}, Tq[3] = {0.0f, 0.0f, 0.0f};
    for (int k = CPF * f; k < CPF * f + CPF; ++k) {
        float fk[3], a[3], r[3], t[3];
        corner_force(M, warm, k, fk);
        for (int i = 0; i < 3; ++i) a[i] = M.foot_pos[k][i] - S.pos[i];
        dwb::m3v(R, a, r);
        dwb::cross(r, fk, t);
        for (int i = 0; i < 3; ++i) { F[i] += fk[i]; Tq[i] += t[i]; }
    }
    if (S.world_frame) {
        for (int i = 0; i < 3; ++i) { out[i] = F[i]; out[3 + i] = Tq[i]; }
        return;
    }
    float Rs[9], a[3], b[3];
    dwb::quat_to_mat(S.quat, Rs);
    m3tv(R, F, a);
    m3tv(Rs, a, out);
    m3tv(R, Tq, b);
    m3tv(Rs, b, out + 3);
}

// cop row [4] of sole f, in the foot frame
DWF_HD void cop_row(const DwfModel &M, int f, const float *warm, float *out) {
    float sx = 0.0f, sy = 0.0f, sn = 0.0f, cnt = 0.0f;
    for (int k = CPF * f; k < CPF * f + CPF; ++k) {
        const float n = warm[3 * k + 2] * M.inv_dt;
        sx += n * M.foot_pos[k][0];
        sy += n * M.foot_pos[k][1];
        sn += n;
        cnt += n > 0.0f ? 1.0f : 0.0f;
    }
    const bool on = sn > 0.0f;
    out[0] = on ? sx / sn : 0.0f;
    out[1] = on ? sy / sn : 0.0f;
    out[2] = on ? sn : 0.0f;
    out[3] = on ? cnt : 0.0f;
}

// corner k's offset from the base: o_f + R_f c_k
DWF_HD void corner_off(const DwfModel &M, const float *fps, int k, float *o) {
    const float *fp = fps + (k / CPF) * FP;
    float r[3];
    dwb::m3v(fp + 3, M.foot_pos[k], r);
    for (int i = 0; i < 3; ++i) o[i] = fp[i] + r[i];
}

// zmp row [4]
DWF_HD void zmp_row(const DwfModel &M, const float *fps, const float *warm, const float *root, float *out) {
    float sx = 0.0f, sy = 0.0f, sn = 0.0f, cnt = 0.0f;
    for (int k = 0; k < NC; ++k) {
        const float n = warm[3 * k + 2] * M.inv_dt;
        float o[3];
        corner_off(M, fps, k, o);
        sx += n * o[0];
        sy += n * o[1];
        sn += n;
        cnt += n > 0.0f ? 1.0f : 0.0f;
    }
    const bool on = sn > 0.0f;
    out[0] = on ? root[0] + sx / sn : 0.0f;
    out[1] = on ? root[1] + sy / sn : 0.0f;
    out[2] = on ? sn : 0.0f;
    out[3] = on ? cnt : 0.0f;
}

// corner row [6]: p_k (the base added last), f_k
DWF_HD void corner_row(const DwfModel &M, int k, const float *fps, const float *warm, const float *root, float *out) {
    float o[3];
    corner_off(M, fps, k, o);
    for (int i = 0; i < 3; ++i) out[i] = root[i] + o[i];
    corner_force(M, warm, k, out + 3);
}

// ---- host: the checks of dwf_refresh that need no device (NULL: fine) ----
inline const char *refusal(const DwfModel *M, const DwfSensor *S, int ns) {
    if (!M) return "the model is missing";
    if (ns < 0 || ns > NS) return "ns must be in 0..8";
    if (ns > 0 && !S) return "the sensor array is missing";
    if (!isfinite(M->inv_dt)) return "inv_dt is not finite";
    for (int f = 0; f < DWF_NUM_FEET; ++f)
        if (M->foot_mv[f] < 1 || M->foot_mv[f] > DWF_LEG_DOF) return "a foot_mv is outside 1..12";
    for (int s = 0; s < ns; ++s) {
        if (S[s].foot < 0 || S[s].foot > 1) return "a sensor's foot is outside 0..1";
        const float *q = S[s].quat;
        const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (!(n >= 0.99f && n <= 1.01f)) return "a sensor's quaternion has a norm outside [0.99, 1.01]";
    }
    return nullptr;
}

}  // namespace dwf

#endif
