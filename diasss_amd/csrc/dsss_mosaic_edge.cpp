// diasss_amd/csrc/dsss_mosaic_edge.cpp -- the host arithmetic of the overlap registration (include/dsss.h, section "mosaic"): what
// launches nothing and holds no device code.  The peak of a table on the host (peak_of: the one body of dsss_mosaic_int.h, as
// mosaic_peak_kernel applies it on the device), the yaw fan's angles, rotation and angle rule, the pyramid's level rule, a segment
// row as a pose-graph edge (edge_of) and the row loop of the two edges entries, with their public wrappers and the defaults of the
// parameter structs.  The kernels and the orchestration of the four registration entries are in dsss_mosaic_reg.hip; the few
// functions it needs from here are declared in dsss_mosaic_int.h.
#include "dsss_mosaic_int.h"
#include "dsss_pose.h"
#include <algorithm>

int peak_of(const uint64_t* sums, int radius, int min_cells, double cell, dsss_reg_result* out)
{
    const int S = 2 * radius + 1;
    std::vector<reg_score> z((size_t)S * S);
    for (int s = 0; s < S * S; ++s) z[s] = reg_score_of(sums + (size_t)s * 6, min_cells);
    bool found = false; int bx = 0, by = 0;
    for (int dy = -radius; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) {
            const reg_score& q = z[(size_t)(dy + radius) * S + (dx + radius)];
            if (!q.ok) continue;
            if (!found || reg_better(q.z, dx, dy, z[(size_t)(by + radius) * S + (bx + radius)].z, bx, by)) { found = true; bx = dx; by = dy; }
        }
    const size_t zero = (size_t)radius * S + radius, pk = (size_t)(by + radius) * S + (bx + radius);
    const bool inner = found && abs(bx) != radius && abs(by) != radius;      // the four neighbours exist
    const reg_score none = { -2.0, false };
    reg_record(found, bx, by, radius, cell, z[zero], sums[zero * 6], z[pk], sums[pk * 6], inner ? z[pk - 1] : none, inner ? z[pk + 1] : none,
               inner ? z[pk - S] : none, inner ? z[pk + S] : none, out);
    return DSSS_OK;
}

// ---- the yaw fan
bool fan_ok(int nyaw, double step) { return nyaw >= 1 && nyaw <= REG_MAX_YAW && (nyaw & 1) && step > 0.0 && std::isfinite(step); }
double fan_theta(int k, int nyaw, double step) { return (double)(k - (nyaw - 1) / 2) * step; }

// the pings [p0, p1) of rows_b rotated by theta about the position of ping (p0 + p1) / 2 -> out, (p1 - p0) x 6
void rotate_rows(const double* rows_b, int p0, int p1, double theta, double* out)
{
    const double* piv = rows_b + (size_t)(((long long)p0 + p1) / 2) * 6;
    double s, co; dsss_sincos(theta, &s, &co);
    for (int i = p0; i < p1; ++i) dsss_rotate_row(rows_b + (size_t)i * 6, piv[3], piv[4], theta, s, co, out + (size_t)(i - p0) * 6);
}

// the angle rule of the header, "dense loop closures with a yaw fan": the one place it is written
void yaw_peak_of(const dsss_reg_result* z, int nyaw, double step, int32_t* k, int32_t* border, double* theta, double* theta_hat)
{
    const int mid = (nyaw - 1) / 2;
    int best = -1;
    for (int i = 0; i < nyaw; ++i) {
        if (!(z[i].zncc > -2.0)) continue;
        if (best < 0 || z[i].zncc > z[best].zncc || (z[i].zncc == z[best].zncc && abs(i - mid) < abs(best - mid))) best = i;   // equals at one distance: the lower k came first
    }
    if (best < 0) { *k = mid; *border = 0; *theta = 0.0; *theta_hat = 0.0; return; }
    *k = best; *border = (nyaw > 1 && (best == 0 || best == nyaw - 1)) ? 1 : 0;
    *theta = fan_theta(best, nyaw, step);
    double q = 0.0;
    if (!*border && nyaw > 1 && z[best - 1].zncc > -2.0 && z[best + 1].zncc > -2.0) {
        const double zm = z[best - 1].zncc, z0 = z[best].zncc, zp = z[best + 1].zncc;
        const double den = zm - 2.0 * z0 + zp;
        if (den < 0.0) q = 0.5 * (zm - zp) / den;
    }
    *theta_hat = *theta + q * step;
}

// ---- the cell pyramid
bool pyr_ok(const dsss_reg_pyr_params& P) { return P.levels >= 1 && P.levels <= PYR_MAX_LEVELS && (P.levels == 1 || (P.refine >= 1 && P.refine <= REG_MAX_RADIUS)); }

// the level rule of the header, "dense loop closures over a cell pyramid": the one place it is written.  sums = the table of level
// `level` around the centre (cx, cy); min_cells and cell are the level-0 values.  It has two parts: the record of the level's table
// under pyr_min_cells and the level's cell (peak_of on the host, mosaic_peak_kernel on the device), and pyr_centre_of, which adds the
// centre to that record (*out) and is host arithmetic on both paths.
void pyr_centre_of(double cell, int level, int cx, int cy, dsss_reg_result* out, int32_t* usable, int32_t* ncx, int32_t* ncy)
{
    const double cell_l = ldexp(cell, level);
    *usable = out->zncc > -2.0 ? 1 : 0;
    if (!*usable) return;                                                       // the no-usable-shift record as it is: no centre is added to it
    out->dx += cx; out->dy += cy;
    const double mx = (double)cx * cell_l, my = (double)cy * cell_l;            // one multiply and one add each, unfused (-ffp-contract=off)
    out->off_x = out->off_x + mx; out->off_y = out->off_y + my;
    if (level > 0) { *ncx = 2 * out->dx; *ncy = 2 * out->dy; }
}
int pyr_min_cells(int min_cells, int level) { return std::max(1, min_cells >> (2 * level)); }
static void pyr_step_of(const uint64_t* sums, int radius, int min_cells, double cell, int level, int cx, int cy, dsss_reg_result* out, int32_t* usable,
                 int32_t* ncx, int32_t* ncy)
{
    peak_of(sums, radius, pyr_min_cells(min_cells, level), ldexp(cell, level), out);
    pyr_centre_of(cell, level, cx, cy, out, usable, ncx, ncy);
}

namespace {

// dsss_register_edge and dsss_register_edge_yaw: the segment row s as an edge, its pings rotated by theta where the anchor ping is
// looked for and by theta_hat where it is measured (both 0: the rows as they are), s_yaw = the sigma of the yaw
int edge_of(const dsss_reg_seg* s, const dsss_mosaic_params* grid, const double* rows_a, int Na, int base_a, const double* rows_b, int Nb, int base_b,
            const dsss_reg_edge_params& E, double theta, double theta_hat, double s_yaw, dsss_lc_edge* edge)
{
    if (!s || !grid || !rows_a || !rows_b || !edge || Na < 1 || Nb < 1) return DSSS_E_ARG;
    if (s->p0 < 0 || s->p0 >= s->p1 || s->p1 > Nb) return DSSS_E_ARG;
    if (!(grid->cell > 0.0) || !std::isfinite(grid->cell)) return DSSS_E_ARG;
    const double sig[4] = { E.sigma_xy_cells, E.sigma_z, E.sigma_rot, s_yaw };
    for (double v : sig) if (!(v > 0.0) || !std::isfinite(v)) return DSSS_E_ARG;
    if (!std::isfinite(theta) || !std::isfinite(theta_hat)) return DSSS_E_ARG;
    if (!(s->r.zncc >= E.min_zncc) || s->r.on_border != 0) return 0;
    if (s->r.n <= 0) return DSSS_E_ARG;
    const double cell = grid->cell;
    const double cx = grid->x0 + ((double)s->sx / (double)s->r.n + 0.5) * cell, cy = grid->y0 + ((double)s->sy / (double)s->r.n + 0.5) * cell;
    // the ping whose scan line (through the ping, across the heading) passes nearest the point: the lowest index among equals
    auto anchor = [](const double* rows, int r0, int r1, double px, double py) {
        int best = r0; double dbest = INFINITY;
        for (int i = r0; i < r1; ++i) {
            const double* P = rows + (size_t)i * 6;
            const double d = fabs(cos(P[2]) * (px - P[3]) + sin(P[2]) * (py - P[4]));
            if (d < dbest) { dbest = d; best = i; }
        }
        return best;
    };
    const int i = anchor(rows_a, 0, Na, cx, cy);
    std::vector<double> rot((size_t)(s->p1 - s->p0) * 6);                       // the segment's rows under theta (theta == 0: a copy)
    rotate_rows(rows_b, s->p0, s->p1, theta, rot.data());
    const int j = s->p0 + anchor(rot.data(), 0, s->p1 - s->p0, cx + s->r.off_x, cy + s->r.off_y);      // b's rendering lies off from where it belongs
    double rowj[6], sh, ch;                                                     // row j of the rows under theta_hat
    const double* piv = rows_b + (size_t)(((long long)s->p0 + s->p1) / 2) * 6;
    dsss_sincos(theta_hat, &sh, &ch);
    dsss_rotate_row(rows_b + (size_t)j * 6, piv[3], piv[4], theta_hat, sh, ch, rowj);
    pose_t Xa, Xb, rel;
    pose_from_rodrigues(rows_a + (size_t)i * 6, &Xa);
    pose_from_rodrigues(rowj, &Xb);
    Xb.t[0] -= s->r.off_x; Xb.t[1] -= s->r.off_y;
    const long long ga = (long long)base_a + i, gb = (long long)base_b + j;
    if (ga < 0 || gb < 0 || ga > 0x7fffffffll || gb > 0x7fffffffll) return DSSS_E_ARG;
    if (ga < gb) { edge->a = (int32_t)ga; edge->b = (int32_t)gb; pose_between(&Xa, &Xb, &rel); }
    else { edge->a = (int32_t)gb; edge->b = (int32_t)ga; pose_between(&Xb, &Xa, &rel); }
    memcpy(edge->rel, rel.R, 9 * sizeof(double)); memcpy(edge->rel + 9, rel.t, 3 * sizeof(double));
    const double sxy = E.sigma_xy_cells * cell;
    edge->var[0] = edge->var[1] = E.sigma_rot * E.sigma_rot; edge->var[2] = s_yaw * s_yaw;
    edge->var[3] = edge->var[4] = sxy * sxy; edge->var[5] = E.sigma_z * E.sigma_z;
    return 1;
}

// the row loop of dsss_mosaic_register_edges and dsss_mosaic_register_edges_yaw: seg_of(k) = the (pair, segment) part of row k,
// edge_fn(k, rows_a, Na, base_a, rows_b, Nb, base_b, &e) = what dsss_register_edge(_yaw) says about it
template <class SegOf, class EdgeFn>
int edges_loop(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p, const int* pair_a, const int* pair_b,
               bool have_segs, int nsegs, dsss_lc_edge* edges_host, int32_t* edge_seg_host, int cap, int* n_edges, SegOf seg_of, EdgeFn edge_fn)
{
    if (!c) return DSSS_E_ARG;
    if (dsss_comm_world(c) > 1) DSSS_FAIL(c, DSSS_E_STATE, "mosaic: registration runs on a single rank (communicator of %d)", dsss_comm_world(c));
    size_t rows = 0;
    int rc = mosaic_check_frames(c, ids, n, rpy6, ping_off, false, &rows); if (rc) return rc;
    rc = mosaic_check_params(c, p); if (rc) return rc;
    if (nsegs < 0 || cap < 0 || !n_edges) DSSS_FAIL(c, DSSS_E_ARG, "register: nsegs = %d, cap = %d%s", nsegs, cap, n_edges ? "" : ", nowhere to write the number of edges");
    if (nsegs > 0 && (!pair_a || !pair_b || !have_segs)) DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments without %s", nsegs, have_segs ? "their pairs" : "their rows");
    std::vector<int> slot(c->max_frames, -1), base(n);
    int run = 0;
    for (int i = 0; i < n; ++i) { slot[ids[i]] = i; base[i] = ping_off ? ping_off[i] : run; run += c->frames[ids[i]].N; }
    int ne = 0;
    for (int k = 0; k < nsegs; ++k) {
        const dsss_reg_seg& sg = seg_of(k);
        if (sg.pair < 0) DSSS_FAIL(c, DSSS_E_ARG, "register: row %d names pair %d", k, sg.pair);
        const int a = pair_a[sg.pair], b = pair_b[sg.pair];
        if (a < 0 || a >= c->max_frames || slot[a] < 0 || b < 0 || b >= c->max_frames || slot[b] < 0)
            DSSS_FAIL(c, DSSS_E_ARG, "register: row %d, pair (%d, %d) names a frame that is not listed", k, a, b);
        const int ia = slot[a], ib = slot[b];
        const dsss_frame& fa = c->frames[a]; const dsss_frame& fb = c->frames[b];
        dsss_lc_edge e;
        rc = edge_fn(k, rpy6 ? rpy6 + (size_t)ping_off[ia] * 6 : fa.h_geo, fa.N, base[ia],
                     rpy6 ? rpy6 + (size_t)ping_off[ib] * 6 : fb.h_geo, fb.N, base[ib], &e);
        if (rc < 0) DSSS_FAIL(c, rc, "register: row %d (pair %d, segment %d, pings %d..%d) is not a valid segment result", k, sg.pair, sg.seg, sg.p0, sg.p1);
        if (rc == 0) continue;
        if (ne >= cap || !edges_host) DSSS_FAIL(c, DSSS_E_CAPACITY, "register: more than %d edges", edges_host ? cap : 0);
        edges_host[ne] = e;
        if (edge_seg_host) edge_seg_host[ne] = k;
        ++ne;
    }
    *n_edges = ne;
    return DSSS_OK;
}

} // namespace

extern "C" {

void dsss_reg_params_default(dsss_reg_params* p) { if (p) { p->radius = 8; p->min_cells = 256; } }

int dsss_mosaic_register_peak(const uint64_t* sums, int radius, int min_cells, double cell, dsss_reg_result* out)
{
    if (!sums || !out || radius < 0 || radius > REG_MAX_RADIUS || min_cells < 1 || !(cell > 0.0) || !std::isfinite(cell)) return DSSS_E_ARG;
    return peak_of(sums, radius, min_cells, cell, out);
}

void dsss_reg_edge_params_default(dsss_reg_edge_params* e) { if (e) { e->min_zncc = 0.5; e->sigma_xy_cells = 1.0; e->sigma_z = 10.0; e->sigma_rot = 1.0; } }

int dsss_register_edge(const dsss_reg_seg* s, const dsss_mosaic_params* grid, const double* rows_a, int Na, int base_a,
                       const double* rows_b, int Nb, int base_b, const dsss_reg_edge_params* ep, dsss_lc_edge* edge)
{
    dsss_reg_edge_params E; dsss_reg_edge_params_default(&E);
    if (ep) E = *ep;
    return edge_of(s, grid, rows_a, Na, base_a, rows_b, Nb, base_b, E, 0.0, 0.0, E.sigma_rot, edge);
}

int dsss_mosaic_register_edges(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                               const int* pair_a, const int* pair_b, const dsss_reg_seg* segs, int nsegs, const dsss_reg_edge_params* ep,
                               dsss_lc_edge* edges_host, int32_t* edge_seg_host, int cap, int* n_edges)
{
    return edges_loop(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, segs != nullptr, nsegs, edges_host, edge_seg_host, cap, n_edges,
                      [&](int k) -> const dsss_reg_seg& { return segs[k]; },
                      [&](int k, const double* ra, int Na, int ba, const double* rb, int Nb, int bb, dsss_lc_edge* e) {
                          return dsss_register_edge(segs + k, p, ra, Na, ba, rb, Nb, bb, ep, e); });
}

// ---- dense loop closures with a yaw fan
void dsss_reg_yaw_params_default(dsss_reg_yaw_params* y) { if (y) { y->nyaw = 1; y->pad_ = 0; y->step = 0.01; } }

int dsss_register_rotate_rows(const double* rows_b, int Nb, int p0, int p1, double theta, double* out)
{
    if (!rows_b || !out || p0 < 0 || p0 >= p1 || p1 > Nb || !std::isfinite(theta)) return DSSS_E_ARG;
    rotate_rows(rows_b, p0, p1, theta, out);
    return DSSS_OK;
}

int dsss_register_yaw_peak(const dsss_reg_result* per_angle, int nyaw, double step, int32_t* k, int32_t* yaw_on_border, double* theta, double* theta_hat)
{
    if (!per_angle || !k || !yaw_on_border || !theta || !theta_hat || !fan_ok(nyaw, step)) return DSSS_E_ARG;
    yaw_peak_of(per_angle, nyaw, step, k, yaw_on_border, theta, theta_hat);
    return DSSS_OK;
}

void dsss_reg_edge_yaw_params_default(dsss_reg_edge_yaw_params* e)
{
    if (e) { dsss_reg_edge_params_default(&e->e); dsss_reg_yaw_params_default(&e->fan); e->sigma_yaw_steps = 1.0; }
}

int dsss_register_edge_yaw(const dsss_reg_seg_yaw* s, const dsss_mosaic_params* grid, const double* rows_a, int Na, int base_a,
                           const double* rows_b, int Nb, int base_b, const dsss_reg_edge_yaw_params* ep, dsss_lc_edge* edge)
{
    dsss_reg_edge_yaw_params E; dsss_reg_edge_yaw_params_default(&E);
    if (ep) E = *ep;
    if (!s || !fan_ok(E.fan.nyaw, E.fan.step) || !(E.sigma_yaw_steps > 0.0) || !std::isfinite(E.sigma_yaw_steps)) return DSSS_E_ARG;
    const double s_yaw = E.fan.nyaw == 1 ? E.e.sigma_rot : E.sigma_yaw_steps * E.fan.step;
    // the row's own acceptance comes first in edge_of; a fan row on the border of the fan is rejected after it was found valid
    dsss_lc_edge e;
    const int rc = edge_of(&s->s, grid, rows_a, Na, base_a, rows_b, Nb, base_b, E.e, s->theta, s->theta_hat, s_yaw, edge ? &e : nullptr);
    if (rc != 1) return rc;
    if (s->yaw_on_border != 0) return 0;
    *edge = e;
    return 1;
}

int dsss_mosaic_register_edges_yaw(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                                   const int* pair_a, const int* pair_b, const dsss_reg_seg_yaw* segs, int nsegs, const dsss_reg_edge_yaw_params* ep,
                                   dsss_lc_edge* edges_host, int32_t* edge_seg_host, int cap, int* n_edges)
{
    return edges_loop(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, segs != nullptr, nsegs, edges_host, edge_seg_host, cap, n_edges,
                      [&](int k) -> const dsss_reg_seg& { return segs[k].s; },
                      [&](int k, const double* ra, int Na, int ba, const double* rb, int Nb, int bb, dsss_lc_edge* e) {
                          return dsss_register_edge_yaw(segs + k, p, ra, Na, ba, rb, Nb, bb, ep, e); });
}

// ---- dense loop closures over a cell pyramid
void dsss_reg_pyr_params_default(dsss_reg_pyr_params* q) { if (q) { q->levels = 1; q->refine = 3; } }

int dsss_register_pyr_step(const uint64_t* sums, int radius, int min_cells, double cell, int level, int cx, int cy,
                           dsss_reg_result* out, int32_t* usable, int32_t* ncx, int32_t* ncy)
{
    if (!sums || !out || !usable || !ncx || !ncy || radius < 0 || radius > REG_MAX_RADIUS || min_cells < 1 || !(cell > 0.0) || !std::isfinite(cell) ||
        level < 0 || level >= PYR_MAX_LEVELS || cx < -PYR_MAX_CENTRE || cx > PYR_MAX_CENTRE || cy < -PYR_MAX_CENTRE || cy > PYR_MAX_CENTRE) return DSSS_E_ARG;
    pyr_step_of(sums, radius, min_cells, cell, level, cx, cy, out, usable, ncx, ncy);
    return DSSS_OK;
}

} // extern "C"
