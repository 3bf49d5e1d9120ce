// What the kernels of a second component read about the engine: k_template (lcf_template.hip, the likelihood and the
// component evaluation) and k_tq_pass / k_tq_features (lcf_predict.hip, the bands and features of such a fit).
#pragma once

#include "lcf_internal.h"

// (An unnamed namespace in a header, on purpose: the kernels that take the struct by value have internal linkage in their
// own files, and their symbols -- which carry the parameter's type -- stay what they were when the struct lived in
// lcf_template.hip.)
namespace {

struct TemplateDev {
    int n_points, n_knots, n_dim, use_sigma, sigma_abs, i_tmax, i_s, pad;
    double unit_abs, log_norm_const, inv_h;
    const double *knots, *coef, *t, *y, *dy;   // the photometry in the caller's order, as m is
    const int *filt, *fac, *off;               // per point: its filter; per filter: the columns of its r and dt, -1: none
};

inline TemplateDev template_dev(const lcf_engine* e) {
    const DevProblem& pb = e->dp;
    TemplateDev a{};
    a.n_points = pb.n_points, a.n_knots = e->tpl_nk, a.n_dim = pb.n_dim, a.use_sigma = pb.use_sigma;
    a.sigma_abs = pb.sigma_abs, a.i_tmax = e->tpl_tmax, a.i_s = e->tpl_s;
    a.unit_abs = pb.sigma_unit_abs, a.log_norm_const = pb.log_norm_const, a.inv_h = e->tpl_inv_h;
    a.knots = e->tpl_knots, a.coef = e->tpl_coef, a.t = e->tpl_t, a.y = e->tpl_y, a.dy = e->tpl_dy;
    a.filt = e->tpl_filt, a.fac = e->tpl_fac, a.off = e->tpl_off;
    return a;
}

}  // namespace
