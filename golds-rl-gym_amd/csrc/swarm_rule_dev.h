// The feedback rule of the Swarm env (include/goldsrl_swarmrules.h), shared by the translation units that act by it (swarm_rules.hip:
// whole episodes per rule; swarm_plan.hip: the receding-horizon planner over the same table; swarm_search.hip: the search over a rule's
// numbers): the device statements of one action
// and the host's checks of a rule table.  One copy, so the two entry points cannot drift apart in a rounding or a refusal.
// Every including file is compiled with -ffp-contract=off.
#pragma once
#include <math.h>

#include <string>

#include "common.h"
#include "swarm_dev.h"

namespace grl {

// The action of agent a of one pair from the pair's points as they stand before the step: pts[0..79] the locusts, pts[80 + a] the
// agent.  Each statement is one rounding.
__device__ __forceinline__ void rule_action(const double2 *pts, int a, double cancel, double gain, int anchor, double offx, double offy,
                                            double &ax, double &ay) {
    const double2 me = pts[N_LOCUSTS + a];
    double cx, cy;
    if (anchor == 0) {             // the centroid: a sequential sum, index order
        cx = 0.0;
        cy = 0.0;
#pragma unroll 8
        for (int j = 0; j < N_LOCUSTS; ++j) {
            const double2 q = pts[j];
            cx = cx + q.x;
            cy = cy + q.y;
        }
        cx = cx / 80.0;
        cy = cy / 80.0;
    } else {                       // the nearest locust: strict <, so the first index wins a tie
        double best;
        {
            const double2 q = pts[0];
            const double dx = q.x - me.x, dy = q.y - me.y;
            const double sx = dx * dx, sy = dy * dy;
            best = sx + sy;
            cx = q.x;
            cy = q.y;
        }
#pragma unroll 8
        for (int j = 1; j < N_LOCUSTS; ++j) {
            const double2 q = pts[j];
            const double dx = q.x - me.x, dy = q.y - me.y;
            const double sx = dx * dx, sy = dy * dy;
            const double d2 = sx + sy;
            if (d2 < best) {
                best = d2;
                cx = q.x;
                cy = q.y;
            }
        }
    }
    const double tx = cx + offx, ty = cy + offy;
    const double ex = tx - me.x, ey = ty - me.y;
    const double gx = gain * ex;
    ax = gx - cancel;
    ay = gain * ey;
    const double qx = ax * ax, qy = ay * ay;
    const double d = sqrt(qx + qy);
    if (d >= 1.0) {                // transform_actions_for_env: a row of norm >= 1 is divided by its norm
        ax = ax / d;
        ay = ay / d;
    }
}

// The host's checks of a rule table: rules (n_rules, 3) rows (cancel, gain, anchor), offsets (n_rules, 10, 2).  fn: the C
// function's name, with which every message starts.
static int swarm_check_rule_table(grl_handle *h, const char *fn, const double *rules_host, const double *offsets_host, int n_rules) {
    const std::string f = std::string(fn) + ": rule ";
    for (int i = 0; i < n_rules; ++i) {
        const double *r = rules_host + (size_t)i * 3;
        if (!std::isfinite(r[0]) || !std::isfinite(r[1])) return fail(h, GRL_E_INVALID, f + std::to_string(i) + ": cancel or gain is not finite");
        if (!(r[2] == 0.0 || r[2] == 1.0))
            return fail(h, GRL_E_INVALID, f + std::to_string(i) + ": anchor must be 0 (centroid) or 1 (nearest locust)");
        for (int k = 0; k < N_AGENTS * 2; ++k)
            if (!std::isfinite(offsets_host[(size_t)i * N_AGENTS * 2 + k]))
                return fail(h, GRL_E_INVALID, f + std::to_string(i) + ": an offset is not finite");
    }
    return GRL_OK;
}

// a checked table onto the device, on the handle's stream
static int swarm_upload_rule_table(grl_handle *h, double *rules, double *offsets, const double *rules_host, const double *offsets_host, size_t n_rules) {
    GRL_HIP(h, hipMemcpyAsync(rules, rules_host, n_rules * 3 * 8, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemcpyAsync(offsets, offsets_host, n_rules * N_AGENTS * 2 * 8, hipMemcpyHostToDevice, h->stream));
    return GRL_OK;
}

}  // namespace grl
