// numerics.cpp — host entry points of the shared 3x3 numerics (numerics.hpp).
#include "pcr_internal.hpp"
#include "numerics.hpp"
#include "kabsch_wave.hpp"

#include <cmath>

namespace pcr {

void svd3(const double A[9], double U[9], double S[3], double V[9]) { num::svd3(A, U, S, V); }

int kabsch_solve(const double sums[16], float R[9], float t[3])
{
    return num::kabsch_solve(sums, R, t) == 0 ? PCR_OK : PCR_ERR_EMPTY;
}

int kabsch_solve_lanes(const double sums[16], float R[9], float t[3])
{
    const int rc = num::kabsch_solve_host_lanes(sums, R, t);
    return rc == 0 ? PCR_OK : rc == -1 ? PCR_ERR_EMPTY : PCR_ERR_STATE;
}

void mat4_mul_f32(const float A[16], const float B[16], float out[16]) { num::mat4_mul_f32(A, B, out); }

}  // namespace pcr

// ---- small dense real nonsymmetric eigenproblem (Homework3 spectral clustering: the Ritz matrix of csrc/spectral.hip) ----------
// Householder reduction to Hessenberg form, then the shifted (Francis double-step) QR iteration on the Hessenberg matrix with the
// transformations accumulated, and back-substitution for the eigenvectors: the public-domain EISPACK routines orthes / ortran / hqr2, as
// restated in JAMA (NIST).  pcr_eig_small_f64 does no balancing: its matrices are Rayleigh quotients in an orthonormal basis.  eig_dense (the
// Laplacian of a small graph itself, up to 32 rows) runs the permutation half of EISPACK's balanc first: rows and columns that isolate an eigenvalue
// leave the window [low, high] the QR iteration works on, and that eigenvalue is read off the diagonal exactly.  No scaling.
namespace pcr {
namespace {

constexpr int EIG_MAX = 16;
constexpr int EIG_DENSE_MAX = 32;

template <int MAX>
struct EigWork {
    int n, low, high, perm[MAX];
    double H[MAX][MAX], V[MAX][MAX], d[MAX], e[MAX], ort[MAX];
    double cdr, cdi;
    void cdiv(double xr, double xi, double yr, double yi)
    {
        double r, dd;
        if (std::fabs(yr) > std::fabs(yi)) {
            r = yi / yr; dd = yr + r * yi;
            cdr = (xr + r * xi) / dd; cdi = (xi - r * xr) / dd;
        } else {
            r = yr / yi; dd = yi + r * yr;
            cdr = (r * xr + xi) / dd; cdi = (r * xi - xr) / dd;
        }
    }
};

// balanc without its scaling: a row whose off-diagonal entries inside the window are all zero goes to the bottom, such a column to the left
template <class WK>
void eig_isolate(WK& W)
{
    const int n = W.n;
    auto& H = W.H;
    int low = 0, high = n - 1;
    auto exchange = [&](int j, int m) {
        W.perm[m] = j;
        if (j == m) return;
        for (int i = 0; i <= high; i++) { const double t = H[i][j]; H[i][j] = H[i][m]; H[i][m] = t; }
        for (int i = low; i < n; i++) { const double t = H[j][i]; H[j][i] = H[m][i]; H[m][i] = t; }
    };
    for (bool found = true; found && high > 0;) {
        found = false;
        for (int j = high; j >= 0 && !found; j--) {
            bool zero = true;
            for (int i = 0; i <= high && zero; i++) zero = i == j || H[j][i] == 0.0;
            if (zero) { exchange(j, high); high--; found = true; }
        }
    }
    for (bool found = true; found && low < high;) {
        found = false;
        for (int j = low; j <= high && !found; j++) {
            bool zero = true;
            for (int i = low; i <= high && zero; i++) zero = i == j || H[i][j] == 0.0;
            if (zero) { exchange(j, low); low++; found = true; }
        }
    }
    W.low = low; W.high = high;
}

// balbak: the rows of the vectors back to the order of the caller's matrix
template <class WK>
void eig_unpermute(WK& W)
{
    const int n = W.n;
    auto swap_rows = [&](int i) {
        const int k = W.perm[i];
        if (k == i) return;
        for (int j = 0; j < n; j++) { const double t = W.V[i][j]; W.V[i][j] = W.V[k][j]; W.V[k][j] = t; }
    };
    for (int i = W.low - 1; i >= 0; i--) swap_rows(i);
    for (int i = W.high + 1; i < n; i++) swap_rows(i);
}

template <class WK>
void eig_orthes(WK& W)
{
    const int n = W.n, low = W.low, high = W.high;
    auto& H = W.H; auto& V = W.V; auto& ort = W.ort;
    for (int m = low + 1; m <= high - 1; m++) {
        double scale = 0.0;
        for (int i = m; i <= high; i++) scale += std::fabs(H[i][m - 1]);
        if (scale != 0.0) {
            double h = 0.0;
            for (int i = high; i >= m; i--) { ort[i] = H[i][m - 1] / scale; h += ort[i] * ort[i]; }
            double g = std::sqrt(h);
            if (ort[m] > 0) g = -g;
            h -= ort[m] * g;
            ort[m] -= g;
            for (int j = m; j < n; j++) {
                double f = 0.0;
                for (int i = high; i >= m; i--) f += ort[i] * H[i][j];
                f /= h;
                for (int i = m; i <= high; i++) H[i][j] -= f * ort[i];
            }
            for (int i = 0; i <= high; i++) {
                double f = 0.0;
                for (int j = high; j >= m; j--) f += ort[j] * H[i][j];
                f /= h;
                for (int j = m; j <= high; j++) H[i][j] -= f * ort[j];
            }
            ort[m] = scale * ort[m];
            H[m][m - 1] = scale * g;
        }
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int m = high - 1; m >= low + 1; m--) {
        if (H[m][m - 1] != 0.0) {
            for (int i = m + 1; i <= high; i++) ort[i] = H[i][m - 1];
            for (int j = m; j <= high; j++) {
                double g = 0.0;
                for (int i = m; i <= high; i++) g += ort[i] * V[i][j];
                g = (g / ort[m]) / H[m][m - 1];          // double division avoids an underflow
                for (int i = m; i <= high; i++) V[i][j] += g * ort[i];
            }
        }
    }
}

template <class WK>
bool eig_hqr2(WK& W)
{
    const int nn = W.n, low = W.low, high = W.high;
    int n = high;
    auto& H = W.H; auto& V = W.V; auto& d = W.d; auto& e = W.e;
    const double eps = std::ldexp(1.0, -52);
    double exshift = 0.0, p = 0, q = 0, r = 0, s = 0, z = 0, t, w, x, y;
    double norm = 0.0;
    for (int i = 0; i < nn; i++) {
        if (i < low || i > high) { d[i] = H[i][i]; e[i] = 0.0; }          // a root the permutation isolated
        for (int j = (i > 0 ? i - 1 : 0); j < nn; j++) norm += std::fabs(H[i][j]);
    }
    int iter = 0, total = 0;
    while (n >= low) {
        int l = n;
        while (l > low) {
            s = std::fabs(H[l - 1][l - 1]) + std::fabs(H[l][l]);
            if (s == 0.0) s = norm;
            if (std::fabs(H[l][l - 1]) < eps * s) break;
            l--;
        }
        if (l == n) {                                   // one root
            H[n][n] += exshift;
            d[n] = H[n][n]; e[n] = 0.0;
            n--; iter = 0;
        } else if (l == n - 1) {                        // two roots
            w = H[n][n - 1] * H[n - 1][n];
            p = (H[n - 1][n - 1] - H[n][n]) / 2.0;
            q = p * p + w;
            z = std::sqrt(std::fabs(q));
            H[n][n] += exshift;
            H[n - 1][n - 1] += exshift;
            x = H[n][n];
            if (q >= 0) {                               // a real pair
                z = p >= 0 ? p + z : p - z;
                d[n - 1] = x + z;
                d[n] = d[n - 1];
                if (z != 0.0) d[n] = x - w / z;
                e[n - 1] = 0.0; e[n] = 0.0;
                x = H[n][n - 1];
                s = std::fabs(x) + std::fabs(z);
                p = x / s; q = z / s;
                r = std::sqrt(p * p + q * q);
                p /= r; q /= r;
                for (int j = n - 1; j < nn; j++) { z = H[n - 1][j]; H[n - 1][j] = q * z + p * H[n][j]; H[n][j] = q * H[n][j] - p * z; }
                for (int i = 0; i <= n; i++) { z = H[i][n - 1]; H[i][n - 1] = q * z + p * H[i][n]; H[i][n] = q * H[i][n] - p * z; }
                for (int i = low; i <= high; i++) { z = V[i][n - 1]; V[i][n - 1] = q * z + p * V[i][n]; V[i][n] = q * V[i][n] - p * z; }
            } else {                                    // a complex pair
                d[n - 1] = x + p; d[n] = x + p;
                e[n - 1] = z; e[n] = -z;
            }
            n -= 2; iter = 0;
        } else {                                        // no convergence yet: one double step
            x = H[n][n]; y = 0.0; w = 0.0;
            if (l < n) { y = H[n - 1][n - 1]; w = H[n][n - 1] * H[n - 1][n]; }
            if (iter == 10) {                           // Wilkinson's exceptional shift
                exshift += x;
                for (int i = low; i <= n; i++) H[i][i] -= x;
                s = std::fabs(H[n][n - 1]) + std::fabs(H[n - 1][n - 2]);
                x = y = 0.75 * s;
                w = -0.4375 * s * s;
            }
            if (iter == 30) {                           // MATLAB's exceptional shift
                s = (y - x) / 2.0;
                s = s * s + w;
                if (s > 0) {
                    s = std::sqrt(s);
                    if (y < x) s = -s;
                    s = x - w / ((y - x) / 2.0 + s);
                    for (int i = low; i <= n; i++) H[i][i] -= s;
                    exshift += s;
                    x = y = w = 0.964;
                }
            }
            iter++;
            if (++total > 60 * nn) return false;
            int m = n - 2;
            while (m >= l) {
                z = H[m][m];
                r = x - z; s = y - z;
                p = (r * s - w) / H[m + 1][m] + H[m][m + 1];
                q = H[m + 1][m + 1] - z - r - s;
                r = H[m + 2][m + 1];
                s = std::fabs(p) + std::fabs(q) + std::fabs(r);
                p /= s; q /= s; r /= s;
                if (m == l) break;
                if (std::fabs(H[m][m - 1]) * (std::fabs(q) + std::fabs(r)) <
                    eps * (std::fabs(p) * (std::fabs(H[m - 1][m - 1]) + std::fabs(z) + std::fabs(H[m + 1][m + 1])))) break;
                m--;
            }
            for (int i = m + 2; i <= n; i++) {
                H[i][i - 2] = 0.0;
                if (i > m + 2) H[i][i - 3] = 0.0;
            }
            for (int k = m; k <= n - 1; k++) {
                const bool notlast = k != n - 1;
                if (k != m) {
                    p = H[k][k - 1]; q = H[k + 1][k - 1]; r = notlast ? H[k + 2][k - 1] : 0.0;
                    x = std::fabs(p) + std::fabs(q) + std::fabs(r);
                    if (x != 0.0) { p /= x; q /= x; r /= x; }
                }
                if (x == 0.0) break;
                s = std::sqrt(p * p + q * q + r * r);
                if (p < 0) s = -s;
                if (s != 0) {
                    if (k != m) H[k][k - 1] = -s * x;
                    else if (l != m) H[k][k - 1] = -H[k][k - 1];
                    p += s;
                    x = p / s; y = q / s; z = r / s;
                    q /= p; r /= p;
                    for (int j = k; j < nn; j++) {
                        p = H[k][j] + q * H[k + 1][j];
                        if (notlast) { p += r * H[k + 2][j]; H[k + 2][j] -= p * z; }
                        H[k][j] -= p * x;
                        H[k + 1][j] -= p * y;
                    }
                    const int top = n < k + 3 ? n : k + 3;
                    for (int i = 0; i <= top; i++) {
                        p = x * H[i][k] + y * H[i][k + 1];
                        if (notlast) { p += z * H[i][k + 2]; H[i][k + 2] -= p * r; }
                        H[i][k] -= p;
                        H[i][k + 1] -= p * q;
                    }
                    for (int i = low; i <= high; i++) {
                        p = x * V[i][k] + y * V[i][k + 1];
                        if (notlast) { p += z * V[i][k + 2]; V[i][k + 2] -= p * r; }
                        V[i][k] -= p;
                        V[i][k + 1] -= p * q;
                    }
                }
            }
        }
    }
    if (norm == 0.0) return true;
    // back-substitution: the vectors of the upper triangular form
    for (n = nn - 1; n >= 0; n--) {
        p = d[n]; q = e[n];
        if (q == 0) {                                   // a real vector
            int l = n;
            H[n][n] = 1.0;
            for (int i = n - 1; i >= 0; i--) {
                w = H[i][i] - p;
                r = 0.0;
                for (int j = l; j <= n; j++) r += H[i][j] * H[j][n];
                if (e[i] < 0.0) { z = w; s = r; }
                else {
                    l = i;
                    if (e[i] == 0.0) {
                        H[i][n] = w != 0.0 ? -r / w : -r / (eps * norm);
                    } else {                            // solve the real 2 x 2 system
                        x = H[i][i + 1]; y = H[i + 1][i];
                        q = (d[i] - p) * (d[i] - p) + e[i] * e[i];
                        t = (x * s - z * r) / q;
                        H[i][n] = t;
                        H[i + 1][n] = std::fabs(x) > std::fabs(z) ? (-r - w * t) / x : (-s - y * t) / z;
                    }
                    t = std::fabs(H[i][n]);             // overflow control
                    if ((eps * t) * t > 1)
                        for (int j = i; j <= n; j++) H[j][n] /= t;
                }
            }
        } else if (q < 0) {                             // a complex vector: columns n - 1 (real part) and n (imaginary part)
            int l = n - 1;
            if (std::fabs(H[n][n - 1]) > std::fabs(H[n - 1][n])) {
                H[n - 1][n - 1] = q / H[n][n - 1];
                H[n - 1][n] = -(H[n][n] - p) / H[n][n - 1];
            } else {
                W.cdiv(0.0, -H[n - 1][n], H[n - 1][n - 1] - p, q);
                H[n - 1][n - 1] = W.cdr; H[n - 1][n] = W.cdi;
            }
            H[n][n - 1] = 0.0; H[n][n] = 1.0;
            for (int i = n - 2; i >= 0; i--) {
                double ra = 0.0, sa = 0.0, vr, vi;
                for (int j = l; j <= n; j++) { ra += H[i][j] * H[j][n - 1]; sa += H[i][j] * H[j][n]; }
                w = H[i][i] - p;
                if (e[i] < 0.0) { z = w; r = ra; s = sa; }
                else {
                    l = i;
                    if (e[i] == 0) {
                        W.cdiv(-ra, -sa, w, q);
                        H[i][n - 1] = W.cdr; H[i][n] = W.cdi;
                    } else {                            // solve the complex 2 x 2 system
                        x = H[i][i + 1]; y = H[i + 1][i];
                        vr = (d[i] - p) * (d[i] - p) + e[i] * e[i] - q * q;
                        vi = (d[i] - p) * 2.0 * q;
                        if (vr == 0.0 && vi == 0.0) vr = eps * norm * (std::fabs(w) + std::fabs(q) + std::fabs(x) + std::fabs(y) + std::fabs(z));
                        W.cdiv(x * r - z * ra + q * sa, x * s - z * sa - q * ra, vr, vi);
                        H[i][n - 1] = W.cdr; H[i][n] = W.cdi;
                        if (std::fabs(x) > std::fabs(z) + std::fabs(q)) {
                            H[i + 1][n - 1] = (-ra - w * H[i][n - 1] + q * H[i][n]) / x;
                            H[i + 1][n] = (-sa - w * H[i][n] - q * H[i][n - 1]) / x;
                        } else {
                            W.cdiv(-r - y * H[i][n - 1], -s - y * H[i][n], z, q);
                            H[i + 1][n - 1] = W.cdr; H[i + 1][n] = W.cdi;
                        }
                    }
                    t = std::fmax(std::fabs(H[i][n - 1]), std::fabs(H[i][n]));
                    if ((eps * t) * t > 1)
                        for (int j = i; j <= n; j++) { H[j][n - 1] /= t; H[j][n] /= t; }
                }
            }
        }
    }
    // the vectors of the isolated roots, then back to the original coordinates
    for (int i = 0; i < nn; i++)
        if (i < low || i > high)
            for (int j = i; j < nn; j++) V[i][j] = H[i][j];
    for (int j = nn - 1; j >= low; j--)
        for (int i = low; i <= high; i++) {
            z = 0.0;
            for (int k = low; k <= (j < high ? j : high); k++) z += V[i][k] * H[k][j];
            V[i][j] = z;
        }
    return true;
}

}  // namespace

namespace {

template <int MAX>
int eig_run(int n, const double* a, double* wr, double* wi, double* vec, bool isolate)
{
    if (n < 1 || n > MAX || !a || !wr || !wi) return PCR_ERR_ARG;
    for (int i = 0; i < n * n; i++)
        if (!(std::fabs(a[i]) <= 1.79769313486231570815e308)) return PCR_ERR_ARG;
    EigWork<MAX> W;
    W.n = n; W.low = 0; W.high = n - 1;
    for (int i = 0; i < n; i++) {
        W.perm[i] = i;
        for (int j = 0; j < n; j++) W.H[i][j] = a[i * n + j];
    }
    if (isolate) eig_isolate(W);
    eig_orthes(W);
    if (!eig_hqr2(W)) return PCR_ERR_STATE;
    if (isolate) eig_unpermute(W);
    // units (a real root, or a conjugate pair with the positive imaginary part first) in ascending order of the real part; a stable insertion sort
    int start[MAX], len[MAX], units = 0;
    for (int j = 0; j < n;) {
        const int l = W.e[j] != 0.0 ? 2 : 1;
        start[units] = j; len[units] = l; units++;
        j += l;
    }
    for (int u = 1; u < units; u++) {
        const int s = start[u], l = len[u];
        int v = u;
        while (v > 0 && W.d[start[v - 1]] > W.d[s]) { start[v] = start[v - 1]; len[v] = len[v - 1]; v--; }
        start[v] = s; len[v] = l;
    }
    int o = 0;
    for (int u = 0; u < units; u++)
        for (int t = 0; t < len[u]; t++, o++) {
            const int j = start[u] + t;
            wr[o] = W.d[j]; wi[o] = W.e[j];
            if (!vec) continue;
            double sc = 0.0;                            // unit 2-norm (of the complex vector for a pair)
            for (int c = start[u]; c < start[u] + len[u]; c++)
                for (int i = 0; i < n; i++) sc += W.V[i][c] * W.V[i][c];
            sc = sc > 0.0 ? 1.0 / std::sqrt(sc) : 0.0;
            for (int i = 0; i < n; i++) vec[i * n + o] = W.V[i][j] * sc;
        }
    return PCR_OK;
}

}  // namespace

int eig_small(int n, const double* a, double* wr, double* wi, double* vec) { return eig_run<EIG_MAX>(n, a, wr, wi, vec, false); }
int eig_dense(int n, const double* a, double* wr, double* wi, double* vec) { return eig_run<EIG_DENSE_MAX>(n, a, wr, wi, vec, true); }

// the eigengap rule of spectralClustering.cpp:188-197 as written, with eig(i + 1) read only while it exists
int spectral_select_k(const double* eig, int n_eig)
{
    if (!eig || n_eig < 2) return 1;
    const double diff = eig[1] - eig[0];
    for (int i = 1; i + 1 < n_eig; i++) {
        const double temp = eig[i + 1] - eig[i];
        if (temp > 50 * diff) return i + 1;
    }
    return 1;
}

}  // namespace pcr

extern "C" int pcr_eig_small_f64(int n, const double* a, double* wr, double* wi, double* vectors) { return pcr::eig_small(n, a, wr, wi, vectors); }
extern "C" int pcr_spectral_select_k(const double* eigenvalues, int n_eig) { return pcr::spectral_select_k(eigenvalues, n_eig); }
