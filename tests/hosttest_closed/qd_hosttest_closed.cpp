// qd_hosttest_closed.cpp -- CPU-only TEST HARNESS around the __host__ __device__ code of the closed regime (csrc/qd_closed.h):
// the constrained centre, the sector search and the record they leave, at the rows of a caller's voltages, and the open
// search at a caller's centre for comparison.  NOT part of the product.  Built by tests/hosttest_closed/Makefile.
#include <string.h>
#include "qd_closed.h"

// out (each may be null): vpp [n][G], tc [n][N-1], vd [n][N], isa [n], m [n][N], lambda [n], rounds [n], fl [n][N], nvalid [n],
// idx [n][KC] (uint16), E [n][KC] (the record's: * isa, padding included), states [n][KC][N] (zeros from nvalid on), stats [4]
template <int N, int KC>
static int run_closed(const double* par, long n, const double* v_ext, const int32_t* Q, double* vpp_o, double* tc_o, double* vd_o,
                      double* isa_o, double* m_o, double* lam_o, int32_t* rounds_o, int32_t* fl_o, int32_t* nvalid_o, uint16_t* idx_o,
                      double* E_o, int32_t* states_o, unsigned long long* stats) {
    constexpr int G = N + 1, NB = N - 1;
    for (long p = 0; p < n; ++p) {
        double vpp[G], tc[NB], vd[N], ncont[N], isa;
        qd_point_front<N>(par, v_ext + (size_t)p * 2 * N, vpp, tc, vd, ncont, &isa);
        double m[N], lambda;
        const int rounds = qd_closed_centre<N>(par, vd, Q[p], m, &lambda);
        QdPixelRec rec;
        memset(&rec, 0xA5, sizeof(rec));
        double e[KC]; uint16_t id[KC]; double m2[N];
        const int nv = qd_closed_record<N, KC>(par, vd, isa, Q[p], e, 1, id, 1, &rec, m2, stats);
        if (memcmp(m, m2, sizeof(m)) != 0 || nv != rec.nvalid) return 2;
        if (vpp_o) memcpy(vpp_o + (size_t)p * G, vpp, sizeof(vpp));
        if (tc_o) memcpy(tc_o + (size_t)p * NB, tc, sizeof(tc));
        if (vd_o) memcpy(vd_o + (size_t)p * N, vd, sizeof(vd));
        if (isa_o) isa_o[p] = isa;
        if (m_o) memcpy(m_o + (size_t)p * N, m, sizeof(m));
        if (lam_o) lam_o[p] = lambda;
        if (rounds_o) rounds_o[p] = rounds;
        if (fl_o) for (int i = 0; i < N; ++i) fl_o[(size_t)p * N + i] = rec.fl[i];
        if (nvalid_o) nvalid_o[p] = nv;
        for (int k = 0; k < KC; ++k) {
            if (idx_o) idx_o[(size_t)p * KC + k] = rec.idx[k];
            if (E_o) E_o[(size_t)p * KC + k] = rec.E[k];
            if (states_o)
                for (int i = 0; i < N; ++i)
                    states_o[((size_t)p * KC + k) * N + i] = k < nv ? rec.fl[i] + (int)((rec.idx[k] >> (2 * (N - 1 - i))) & 3) - 1 : 0;
        }
    }
    return 0;
}

// the open search (qd_candidates, sorted) at the caller's centre: idx [n][KC], E [n][KC] (* isa; 0 from nvalid on), nvalid [n], fl [n][N]
template <int N, int KC>
static int run_open_at(const double* par, long n, const double* vd, const double* centre, const double* isa, uint16_t* idx_o,
                       double* E_o, int32_t* nvalid_o, int32_t* fl_o) {
    for (long p = 0; p < n; ++p) {
        double e[KC]; uint16_t id[KC]; int32_t fl[N];
        const int nv = qd_candidates<N, KC>(par, vd + (size_t)p * N, centre + (size_t)p * N, e, 1, id, 1, fl, true);
        for (int k = 0; k < KC; ++k) {
            idx_o[(size_t)p * KC + k] = k < nv ? id[k] : 0;
            E_o[(size_t)p * KC + k] = k < nv ? e[k] * isa[p] : 0.0;
        }
        nvalid_o[p] = nv;
        for (int i = 0; i < N; ++i) fl_o[(size_t)p * N + i] = fl[i];
    }
    return 0;
}

#define QDHC_N(F, ...)                                                        \
    switch (N) {                                                              \
        case 2: return F<2, KK>(__VA_ARGS__); case 3: return F<3, KK>(__VA_ARGS__); case 4: return F<4, KK>(__VA_ARGS__);  \
        case 5: return F<5, KK>(__VA_ARGS__); case 6: return F<6, KK>(__VA_ARGS__); case 7: return F<7, KK>(__VA_ARGS__);  \
        case 8: return F<8, KK>(__VA_ARGS__);                                 \
    }                                                                         \
    return 1;
#define QDHC_KC(F, ...)                                                       \
    if (KC == 8) { constexpr int KK = 8; QDHC_N(F, __VA_ARGS__) }             \
    if (KC == 16) { constexpr int KK = 16; QDHC_N(F, __VA_ARGS__) }           \
    if (KC == 32) { constexpr int KK = 32; QDHC_N(F, __VA_ARGS__) }           \
    return 1;

extern "C" int qdhc_closed(int N, int KC, const double* par, long n, const double* v_ext, const int32_t* Q, double* vpp, double* tc,
                           double* vd, double* isa, double* m, double* lambda, int32_t* rounds, int32_t* fl, int32_t* nvalid,
                           uint16_t* idx, double* E, int32_t* states, unsigned long long* stats) {
    QDHC_KC(run_closed, par, n, v_ext, Q, vpp, tc, vd, isa, m, lambda, rounds, fl, nvalid, idx, E, states, stats)
}

extern "C" int qdhc_open_at(int N, int KC, const double* par, long n, const double* vd, const double* centre, const double* isa,
                            uint16_t* idx, double* E, int32_t* nvalid, int32_t* fl) {
    QDHC_KC(run_open_at, par, n, vd, centre, isa, idx, E, nvalid, fl)
}
