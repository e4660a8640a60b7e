// A g++ build of the rigid-body states' per-env arithmetic (isaacgymdyros_amd/csrc/dw_bodies.h) with host pointers: the functions
// dw_bodies.hip runs, driven env by env in the kernel's order (every path of the tree, the records in DWB_LANES strided shares, every output
// word).  tests/test_body_states.py compiles it and holds it against a float64 numpy restatement.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_bodies.h"

extern "C" {

int dwbh_pack_table(const DwbModel *m, uint32_t *table, char *err, int errn) { return dwb::pack(m, table, err, (size_t)errn); }

// states [n][nb][13] and com [n][7], either may be NULL; body_ids NULL: all 38 in order
int dwbh_refresh(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale, const int32_t *body_ids,
                 int nb, int vel_at_com, float *states, float *com) {
    if (n < 1 || !table || !root_states || !dof_state || (!states && !com)) return -1;
    if (!body_ids) nb = dwb::NB;
    if (nb < 1 || nb > dwb::NB) return -1;
    for (int k = 0; body_ids && k < nb; ++k)
        if (body_ids[k] < 0 || body_ids[k] >= dwb::NB) return -1;
    const dwb::Tab T{table};
    for (int e = 0; e < n; ++e) {
        const float *root = root_states + (size_t)e * dwb::IN_ROOT, *dof = dof_state + (size_t)e * dwb::IN_DOF;
        float mvs[dwb::MVW];
        memset(mvs, 0, sizeof(mvs));
        for (int l = 0; l < T.nleaf(); ++l) dwb::walk_path(T, l, root, dof, vel_at_com, mvs);
        if (com) {
            float acc[DWB_COM_WORDS] = {0, 0, 0, 0, 0, 0, 0};
            for (int l = 0; l < DWB_LANES; ++l) {
                float part[DWB_COM_WORDS] = {0, 0, 0, 0, 0, 0, 0};
                dwb::com_part(T, mvs, mass_scale ? mass_scale + (size_t)e * dwb::NB : nullptr, l, DWB_LANES, part);
                for (int i = 0; i < DWB_COM_WORDS; ++i) acc[i] += part[i];
            }
            dwb::com_finish(acc, root, com + (size_t)e * DWB_COM_WORDS);
        }
        if (states)
            for (int k = 0; k < nb; ++k)
                for (int w = 0; w < DWB_ROW; ++w)
                    states[((size_t)e * nb + k) * DWB_ROW + w] = dwb::out_word(T, mvs, root, dwb::row_of(T, body_ids ? body_ids[k] : k), w, vel_at_com);
    }
    return 0;
}

}  // extern "C"
