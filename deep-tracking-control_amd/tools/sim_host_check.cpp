// Stand-alone host check of the argument validation of dtc_sim_step and dtc_sim_step_act, meant to be built with AddressSanitizer on the host side together
// with csrc/sim.hip and csrc/runtime.hip:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer -I include -I csrc \
//         csrc/sim.hip csrc/runtime.hip tools/sim_host_check.cpp -o sim_host_check
// Every call below hands the entry point a bad descriptor and must come back with DTC_ERR_ARG before any HIP call, so the program
// needs no GPU.  Exit status 0: every call was refused (and the sanitizer saw nothing).
#include <cstdio>
#include <cstring>

#include "dtc_hip.h"

static DtcSimCfg good_cfg() {
    DtcSimCfg c;
    std::memset(&c, 0, sizeof c);
    c.num_dof = 12, c.num_bodies = 17, c.num_commands = 4, c.decimation = 4, c.buffer_len = 10, c.resampling_steps = 500;
    for (int l = 0; l < 4; ++l) c.feet[l] = 4 * l + 4, c.thighs[l] = 4 * l + 2;
    c.sim_dt = 0.005f, c.action_scale = 0.25f, c.clip_actions = 100.f, c.joint_inertia = 0.05f, c.contact_eps = 0.005f;
    c.weight = 117.72f, c.r_min = 0.05f, c.rows = 8, c.cols = 8, c.border_size = 20.f, c.horizontal_scale = 0.05f, c.vertical_scale = 0.005f;
    c.lin_vel_x[0] = c.lin_vel_y[0] = -0.75, c.lin_vel_x[1] = c.lin_vel_y[1] = 0.75, c.ang_vel_yaw[0] = -0.5, c.ang_vel_yaw[1] = 0.5;
    c.heading[0] = -3.14, c.heading[1] = 3.14;
    return c;
}

static int failures = 0;
static void refused(const char* what, int rc) {
    const bool ok = rc == DTC_ERR_ARG;
    std::printf("%-40s rc=%d  %s  (%s)\n", what, rc, ok ? "refused" : "NOT REFUSED", dtc_last_error());
    failures += !ok;
}

int main() {
    DtcSimStep* s = new DtcSimStep;                    // on the heap: a read past either struct is the sanitizer's to see
    DtcSimCfg* c = new DtcSimCfg(good_cfg());
    std::memset(s, 0, sizeof *s);
    refused("st == NULL", dtc_sim_step(nullptr, c, 4, nullptr));
    refused("cfg == NULL", dtc_sim_step(s, nullptr, 4, nullptr));
    refused("every required pointer NULL", dtc_sim_step(s, c, 4, nullptr));
    // one required pointer NULL at a time: all 37 pointer members but u_cmd set to a dummy address, then each cleared in turn
    static float dummy[4];
    void** first = reinterpret_cast<void**>(s);
    const size_t n_ptr = sizeof *s / sizeof(void*);
    const size_t u_cmd = offsetof(DtcSimStep, u_cmd) / sizeof(void*), stride0 = offsetof(DtcSimStep, dof_pos_row_stride) / sizeof(void*);
    for (size_t skip = 0; skip < n_ptr; ++skip) {
        if (skip == u_cmd || (skip >= stride0 && skip < stride0 + 4)) continue;
        for (size_t i = 0; i < n_ptr; ++i) first[i] = dummy;
        s->u_cmd = nullptr;
        s->dof_pos_row_stride = s->dof_vel_row_stride = 24, s->dof_pos_elem_stride = s->dof_vel_elem_stride = 2;
        first[skip] = nullptr;
        char what[64];
        std::snprintf(what, sizeof what, "pointer member %zu NULL", skip);
        refused(what, dtc_sim_step(s, c, 4, nullptr));
    }
    for (size_t i = 0; i < n_ptr; ++i) first[i] = dummy;
    s->dof_pos_row_stride = s->dof_vel_row_stride = 24, s->dof_pos_elem_stride = s->dof_vel_elem_stride = 2;
    refused("N == 0", dtc_sim_step(s, c, 0, nullptr));
    refused("N < 0", dtc_sim_step(s, c, -7, nullptr));
    c->num_dof = 65;
    refused("D > 64", dtc_sim_step(s, c, 4, nullptr));
    *c = good_cfg(), c->feet[3] = 17;
    refused("foot body outside the bodies", dtc_sim_step(s, c, 4, nullptr));
    *c = good_cfg(), c->decimation = 0;
    refused("decimation 0", dtc_sim_step(s, c, 4, nullptr));
    *c = good_cfg(), c->rows = 1;
    refused("terrain table of one row", dtc_sim_step(s, c, 4, nullptr));
    *c = good_cfg(), s->dof_pos_row_stride = 8;
    refused("overlapping dof_pos rows", dtc_sim_step(s, c, 4, nullptr));
    int64_t sizes[2] = {0, 0};
    if (dtc_sim_abi_sizes(sizes, 2) != 2 || sizes[0] != (int64_t)sizeof(DtcSimCfg) || sizes[1] != (int64_t)sizeof(DtcSimStep)) ++failures;

    // dtc_sim_step_act: a good descriptor and good constants, then one bad member of DtcSimActuator at a time, with and without tilt
    for (size_t i = 0; i < n_ptr; ++i) first[i] = dummy;
    s->u_cmd = nullptr;
    s->dof_pos_row_stride = s->dof_vel_row_stride = 24, s->dof_pos_elem_stride = s->dof_vel_elem_stride = 2;
    *c = good_cfg();
    DtcSimTilt* tilt = new DtcSimTilt{1.0f, 1e-6f};
    DtcSimActuator* a = new DtcSimActuator;
    const auto good_act = [&] {
        std::memset(a, 0, sizeof *a);
        a->lag_state = dummy, a->push_vel = dummy;
        for (int it = 0; it < 4; ++it) a->lag_choice[it] = (uint8_t)(1 + it);
        a->lag = 1, a->push = 1, a->push_now = 1, a->keep = 0.975f, a->floor2 = 1e-12f, a->push_span = 2.f, a->push_lo = -1.f;
    };
    for (int with_tilt = 0; with_tilt < 2; ++with_tilt) {
        const DtcSimTilt* t = with_tilt ? tilt : nullptr;
        good_act();
        refused("act == NULL", dtc_sim_step_act(s, c, t, nullptr, 4, nullptr));
        refused("act: st == NULL", dtc_sim_step_act(nullptr, c, t, a, 4, nullptr));
        refused("act: cfg == NULL", dtc_sim_step_act(s, nullptr, t, a, 4, nullptr));
        refused("act: N == 0", dtc_sim_step_act(s, c, t, a, 0, nullptr));
        a->lag_state = nullptr;
        refused("lag_state == NULL", dtc_sim_step_act(s, c, t, a, 4, nullptr));
        good_act(), a->push_vel = nullptr;
        refused("push_vel == NULL with pushes configured", dtc_sim_step_act(s, c, t, a, 4, nullptr));
        good_act(), a->lag_choice[0] = 6;
        refused("first lag choice 6", dtc_sim_step_act(s, c, t, a, 4, nullptr));
        good_act(), a->lag_choice[3] = 255;
        refused("last lag choice 255", dtc_sim_step_act(s, c, t, a, 4, nullptr));
        good_act(), a->keep = 0.f;
        refused("keep == 0", dtc_sim_step_act(s, c, t, a, 4, nullptr));
        good_act(), a->keep = 1.0000001f;
        refused("keep > 1", dtc_sim_step_act(s, c, t, a, 4, nullptr));
        good_act(), a->keep = -0.5f;
        refused("keep < 0", dtc_sim_step_act(s, c, t, a, 4, nullptr));
        good_act(), a->floor2 = -1e-12f;
        refused("negative floor", dtc_sim_step_act(s, c, t, a, 4, nullptr));
        good_act(), a->push_span = -2.f;
        refused("negative span", dtc_sim_step_act(s, c, t, a, 4, nullptr));
    }
    good_act(), tilt->max_slope = 0.f;
    refused("act: max_slope == 0", dtc_sim_step_act(s, c, tilt, a, 4, nullptr));
    if (dtc_sim_act_abi_sizes(sizes, 2) != 1 || sizes[0] != (int64_t)sizeof(DtcSimActuator)) ++failures;
    delete a;
    delete tilt;
    delete s;
    delete c;
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
