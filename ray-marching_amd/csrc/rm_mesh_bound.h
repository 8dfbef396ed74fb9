// rm_mesh_bound.h -- what sparse mesh extraction (rm_mesh_sparse.h) knows about a program without running it: a Lipschitz
// bound of map_scene in real arithmetic, and a bound on how far the binary32 evaluation strays from the real value.  Host
// only, no HIP.  DESIGN.md section 15 has the proofs; the rules in short:
//
// Lipschitz bound L (|f(p) - f(q)| <= L |p - q|, Euclidean norm, real arithmetic):
//   Sphere, Box, Cylinder 1 (each is a composition of 1-Lipschitz maps: |.|, max, min, the Euclidean norm, adding constants;
//   true for every sign of the sizes);  Plane |n|;  Union, Subtraction, Intersection, SmoothUnion max(L_a, L_b) (min, max and
//   negation are 1-Lipschitz in the maximum norm of (a, b); the blend's gradient is a convex combination of the operands');
//   Translation and Scale s (value s * child(p / s)) leave L alone;  Rotation (w, a): the position formula is the linear map
//   (1 - 2|a|^2) I + 2 a a^T + 2 w [. x a], which fixes a and scales its normal plane by sqrt((1 - 2|a|^2)^2 + 4 w^2 |a|^2):
//   every leaf below takes the factor max(1, that).  Because the scale cancels exactly it is never multiplied in, so a unit
//   program reports exactly 1.
// Evaluation error E (|computed(p) - f(p)| <= E for every binary32 point p with |p|_inf <= P):
//   forward analysis with u = 2^-24 per rounded operation.  A position carries (m, e): |coordinate| <= m, absolute error
//   <= e; a value carries (v, e) likewise.  Every rule below over-counts the operations.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "rm_decode.h"

struct RmProgramBound {
    double L = 0.0;  // +inf: no bound
    double E = 0.0;  // +inf with L
};

// P: the largest |coordinate| of any point the program will be evaluated at.  Returns rm_decode_program's status.
static inline int rm_program_bound(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, double P, RmProgramBound* out) {
    RmDecoded d;
    const int rc = rm_decode_program(cmd_count, words, n_words, &d);
    if (rc != RM_OK) return rc;
    const double u = 1.0 / 16777216.0, inf = INFINITY;
    struct Pos { double m, e, rot; float s; };  // rot: the product of the rotation factors from the world down to here
    struct Val { double L, v, e; };
    std::vector<Pos> pos{Pos{P, 0.0, 1.0, 1.0f}};
    std::vector<Val> st;
    bool bad = !std::isfinite(P);
    double worst = P;  // the largest magnitude any position or value can reach
    auto param = [&](uint32_t q) {
        float f;
        std::memcpy(&f, words + q, 4);
        if (!std::isfinite(f)) bad = true;
        return (double)f;
    };
    for (uint32_t i = 0, q = 0; i < cmd_count; i++) {
        const uint32_t op = words[q++];
        const Pos cur = pos.back();
        worst = std::fmax(worst, cur.m);
        if (!st.empty()) worst = std::fmax(worst, st.back().v);
        if (op == RM_CMD_TRANSLATION_PUSH) {
            const double t = std::fmax(std::fabs(param(q)), std::fmax(std::fabs(param(q + 1)), std::fabs(param(q + 2))));
            q += 3;
            pos.push_back(Pos{cur.m + t, cur.e + u * (cur.m + t), cur.rot, 1.0f});
        } else if (op == RM_CMD_ROTATION_PUSH) {
            const double w = param(q), ax = param(q + 1), ay = param(q + 2), az = param(q + 3);
            q += 4;
            const double a2 = ax * ax + ay * ay + az * az, a1 = std::fabs(ax) + std::fabs(ay) + std::fabs(az);
            const double sigma = std::sqrt((1.0 - 2.0 * a2) * (1.0 - 2.0 * a2) + 4.0 * w * w * a2);
            // |row sums| of the map as it is computed: p + w * 2 (p x a) + (2 (p x a)) x a
            const double G = 1.0 + 4.0 * std::fabs(w) * a1 + 8.0 * a1 * a1;
            pos.push_back(Pos{G * cur.m, G * cur.e + 16.0 * u * G * cur.m, cur.rot * std::fmax(1.0, sigma), 1.0f});
        } else if (op == RM_CMD_SCALE_PUSH) {
            const double s = std::fabs(param(q));
            if (!(s > 0.0)) bad = true;
            float sf;
            std::memcpy(&sf, words + q, 4);
            q += 1;
            pos.push_back(Pos{cur.m / s, cur.e / s + u * (cur.m / s), cur.rot, sf});
        } else if (op == RM_CMD_TRANSLATION_POP || op == RM_CMD_ROTATION_POP || op == RM_CMD_SCALE_POP) {
            if (op == RM_CMD_SCALE_POP) {
                const double s = std::fabs((double)cur.s);
                Val& t = st.back();
                t.v *= s;
                t.e = t.e * s + u * t.v;
            }
            pos.pop_back();
        } else if (op == RM_CMD_MATERIAL) {
            q += 1;
        } else if (op == RM_CMD_SPHERE || op == RM_CMD_BOX || op == RM_CMD_CYLINDER) {
            const uint32_t np = op == RM_CMD_SPHERE ? 4u : op == RM_CMD_BOX ? 6u : 5u;
            double c = 0.0;
            for (uint32_t k = 0; k < np; k++) c = std::fmax(c, std::fabs(param(q + k)));
            q += np;
            // differences |p - c| <= m + c with error e + u (m + c); sizes subtracted; a norm of at most three of them
            // (relative error < 4 u, |gradient| <= 1 per coordinate), a min / max term, one sum: 4 e + 16 u (m + 2 c) covers it
            const double mag = cur.m + 2.0 * c;
            st.push_back(Val{cur.rot, 2.0 * mag, 4.0 * cur.e + 16.0 * u * mag});
        } else if (op == RM_CMD_PLANE) {
            const double nx = param(q), ny = param(q + 1), nz = param(q + 2), h = std::fabs(param(q + 3));
            q += 4;
            const double n1 = std::fabs(nx) + std::fabs(ny) + std::fabs(nz), mag = n1 * cur.m + h;
            st.push_back(Val{cur.rot * std::sqrt(nx * nx + ny * ny + nz * nz), mag, n1 * cur.e + 4.0 * u * mag});
        } else {  // a binary operator (the decoder accepted the program)
            double k = 0.0;
            if (op == RM_CMD_SMOOTH_UNION) k = param(q++);
            const Val b = st.back();
            st.pop_back();
            Val& a = st.back();
            a.L = std::fmax(a.L, b.L);
            a.e = std::fmax(a.e, b.e);
            a.v = std::fmax(a.v, b.v);
            if (op == RM_CMD_SMOOTH_UNION && k > 0.0) {
                // h = max(k - |a - b|, 0) / k in [0, 1] with absolute error <= (2 u v + 2 u k) / k + u; h h k / 4 and the
                // final difference add a few roundings of quantities <= k and <= v + k
                a.e += 4.0 * u * a.v + 8.0 * u * k;
                a.v += k;
            }
        }
    }
    RmProgramBound r;
    if (!st.empty()) {
        r.L = st.back().L;
        r.E = st.back().e * 4.0 + 1.0e-30;  // (4: headroom; the floor: underflow)
        // magnitudes whose squares leave binary32's range: the evaluation can overflow, nothing is proven
        worst = std::fmax(worst, st.back().v);
        if (bad || !(r.L < 1.0e15) || !(worst < 1.0e15) || !(r.E < 1.0e15)) r.L = r.E = inf;
    }
    *out = r;
    return RM_OK;
}
