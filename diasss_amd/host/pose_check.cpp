// diasss_amd/host/pose_check.cpp -- the SO(3)/SE(3) algebra of csrc/dsss_pose.h evaluated on the host (the kernels compile the same text).
// Reads a flat binary file of cases and writes every function's outputs; tests/test_pose_algebra_cpu.py compares them bit for bit with
// oracle/orc_pose.c and holds both to the 50-digit reference of tests/pose_algebra_ref.py.  Nothing here judges a number.
// Stand-alone, built with the host sanitizers; needs no GPU and no libdsss.
//     pose_check IN OUT      IN: records of 40 doubles [function id, 39 inputs (unused ones zero)], OUT: 36 doubles per record (unused ones zero)
//     id  function              inputs                  outputs
//      0  so3_exp               w[3]                    R[9]
//      1  so3_log               R[9]                    w[3]
//      2  pose_exp              xi[6]                   T[12]
//      3  pose_log              T[12]                   xi[6]
//      4  pose_between          A[12] B[12]             C[12]
//      5  pose_inverse          A[12]                   B[12]
//      6  pose_compose          A[12] B[12]             C[12]
//      7  pose_adjoint          T[12]                   Ad[36]
//      8  pose_retract          T[12] xi[6]             T'[12]
//      9  pose_rpy              T[12]                   rpy[3]
//     10  pose_from_rodrigues   p[6]                    T[12]
//     11  the Between factor's error, as factor_eval (csrc/dsss_pg_dev.h) chains it: Xa[12] Xb[12] rel[12] -> Log(rel^-1 Xa^-1 Xb)[6]
// A pose is 12 doubles: R row-major, then t.
#include "../csrc/dsss_pose.h"
#include <cstdio>
#include <cstring>
#include <vector>

enum { IN_W = 40, OUT_W = 36 };

static pose_t get_pose(const double* p) { pose_t T; std::memcpy(T.R, p, 9 * sizeof(double)); std::memcpy(T.t, p + 9, 3 * sizeof(double)); return T; }
static void put_pose(const pose_t& T, double* o) { std::memcpy(o, T.R, 9 * sizeof(double)); std::memcpy(o + 9, T.t, 3 * sizeof(double)); }

static bool eval(const double* in, double* out)
{
    const double* a = in + 1;
    pose_t A, B, M, O, H;
    switch ((int)in[0]) {
    case 0: so3_exp(a, out); return true;
    case 1: so3_log(a, out); return true;
    case 2: pose_exp(a, &O); put_pose(O, out); return true;
    case 3: A = get_pose(a); pose_log(&A, out); return true;
    case 4: A = get_pose(a); B = get_pose(a + 12); pose_between(&A, &B, &O); put_pose(O, out); return true;
    case 5: A = get_pose(a); pose_inverse(&A, &O); put_pose(O, out); return true;
    case 6: A = get_pose(a); B = get_pose(a + 12); pose_compose(&A, &B, &O); put_pose(O, out); return true;
    case 7: A = get_pose(a); pose_adjoint(&A, out); return true;
    case 8: A = get_pose(a); pose_retract(&A, a + 12, &O); put_pose(O, out); return true;
    case 9: A = get_pose(a); pose_rpy(&A, out); return true;
    case 10: pose_from_rodrigues(a, &O); put_pose(O, out); return true;
    case 11: A = get_pose(a); B = get_pose(a + 12); M = get_pose(a + 24);
             pose_between(&A, &B, &H); pose_between(&M, &H, &O); pose_log(&O, out); return true;
    }
    return false;
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::printf("usage: pose_check IN OUT\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("pose_check: cannot read %s\n", argv[1]); return 2; }
    std::vector<double> in;
    double rec[IN_W];
    size_t got;
    while ((got = std::fread(rec, sizeof(double), IN_W, f)) == IN_W) in.insert(in.end(), rec, rec + IN_W);
    std::fclose(f);
    if (got != 0) { std::printf("pose_check: %s is not a whole number of records\n", argv[1]); return 2; }
    const size_t n = in.size() / IN_W;
    std::vector<double> out(n * OUT_W, 0.0);
    for (size_t i = 0; i < n; ++i)
        if (!eval(&in[i * IN_W], &out[i * OUT_W])) { std::printf("pose_check: record %zu: unknown function id %g\n", i, in[i * IN_W]); return 1; }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || std::fclose(f) != 0) { std::printf("pose_check: cannot write %s\n", argv[2]); return 2; }
    std::printf("pose_check: ok, %zu records\n", n);
    return 0;
}
