// Dump of everything csrc/fc_precond.hpp builds for one operator (no GPU), in the order fc_setup_krylov calls it: blocks, Jacobi damping,
// Schur complement (+ pin), AMG hierarchy with the aggregate ids of every level, the dense coarsest inverse, K_F and the folded transfer
// operators of V(1,1) and V(2,2).  Built and run by tests/test_precond_model_host.py, which compares every piece with the numpy
// specification tests/support/precond_model.py.
//
//   precond_model_dump <in> <out>
//   in:  int32 N, n_vel, nnz, pin (W dof or -1); double pin_shift; int32 rowptr[N + 1], col[nnz]; double val[nnz]; int32 perm[N]
//   out: records  int32 name length, name, int32 type (0: int32, 1: double), int64 count, data
#include <cstdio>
#include <cstring>
#include <string>

#include "../../flowcontrol_amd/csrc/fc_precond.hpp"

using fcpc::Csr;

static FILE* out;
static void put(const std::string& name, int type, int64_t count, const void* data) {
  const int32_t len = (int32_t)name.size(), t = type;
  std::fwrite(&len, 4, 1, out), std::fwrite(name.data(), 1, name.size(), out), std::fwrite(&t, 4, 1, out), std::fwrite(&count, 8, 1, out);
  if (count) std::fwrite(data, type ? 8 : 4, (size_t)count, out);
}
static void put(const std::string& name, const std::vector<int>& v) { put(name, 0, (int64_t)v.size(), v.data()); }
static void put(const std::string& name, const std::vector<double>& v) { put(name, 1, (int64_t)v.size(), v.data()); }
static void put(const std::string& name, double v) { put(name, 1, 1, &v); }
static void put(const std::string& name, const Csr& M) {
  put(name + ".shape", std::vector<int>{M.nrows, M.ncols}), put(name + ".rp", M.rp), put(name + ".ci", M.ci), put(name + ".v", M.v);
}
template <class T>
static std::vector<T> get(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) throw std::runtime_error("short input");
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  try {
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    const std::vector<int> head = get<int>(in, 4);
    const int N = head[0], n_vel = head[1], nnz = head[2], pin = head[3];
    const double pin_shift = get<double>(in, 1)[0];
    const std::vector<int> rowptr = get<int>(in, (size_t)N + 1), col = get<int>(in, (size_t)nnz);
    const std::vector<double> val = get<double>(in, (size_t)nnz);
    const std::vector<int> perm = get<int>(in, (size_t)N);
    std::fclose(in);
    out = std::fopen(argv[2], "wb");
    if (!out) return 2;

    const fcpc::Blocks X = fcpc::split_blocks(N, n_vel, rowptr, col, val.data(), perm);
    put("vpos", X.vpos), put("ppos", X.ppos), put("F", X.F), put("B", X.B), put("Bt", X.Bt), put("dF", X.dF);
    std::vector<double> dinv((size_t)X.nu), wdinv((size_t)X.nu);
    for (int i = 0; i < X.nu; ++i) dinv[(size_t)i] = 1.0 / X.dF[(size_t)i];
    const double rhoF = fcpc::rho_dinv(X.F, X.dF), omega = std::min(1.0, 1.4 / rhoF);  // (one sweep runs undamped: omega = 1)
    put("rhoF", rhoF), put("omega", omega);
    for (int i = 0; i < X.nu; ++i) wdinv[(size_t)i] = omega * dinv[(size_t)i];
    put("KF", fcpc::fold_jacobi2(X.F, wdinv));
    Csr S = fcpc::spgemm(X.B, X.Bt, dinv.data());
    if (pin >= 0)
      for (int k = 0; k < X.np; ++k)
        if (perm[(size_t)X.ppos[(size_t)k]] == pin)
          for (int q = S.rp[(size_t)k]; q < S.rp[(size_t)k + 1]; ++q)
            if (S.ci[(size_t)q] == k) S.v[(size_t)q] += pin_shift;
    put("S", S);
    const fcpc::Amg H = fcpc::build_amg(S);
    put("levels", std::vector<int>{(int)H.levels.size(), H.n_coarse});
    for (size_t l = 0; l < H.levels.size(); ++l) {
      const fcpc::Level& V = H.levels[l];
      const std::string p = "L" + std::to_string(l) + ".";
      std::vector<int> agg;
      fcpc::aggregate(V.A, 0.08, agg);
      put(p + "agg", agg), put(p + "A", V.A), put(p + "P", V.P), put(p + "R", V.R), put(p + "wdinv", V.wdinv), put(p + "rho", V.rho);
      put(p + "G1", fcpc::fold_down(V)), put(p + "U1", fcpc::fold_up(V));
      Csr G, U;
      fcpc::fold_v22(V, G, U);
      put(p + "G2", G), put(p + "U2", U);
    }
    put("cinv", H.coarse_inv);
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
