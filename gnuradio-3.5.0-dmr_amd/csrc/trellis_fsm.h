// trellis_fsm.h -- host arithmetic of gr-trellis' finite-state machine: fsm (gr-trellis/src/lib/fsm.cc:34-452) and the
// digit helpers of base.cc:29-81, statement for statement in the reference's types.  No device code:
// host/trellis_fsm_test.cc runs it under the sanitizers.  Not part of the ABI.
//
// Where this differs from the reference (include/grhip.h says the same):
//   * the reference validates nothing and indexes out of range; here I, S, O < 1, table lengths other than I * S, an NS
//     entry outside [0, S) and an OS entry outside [0, O) are refused, and so is a file that ends early (the reference
//     leaves the entries unset);
//   * a disconnected FSM is accepted, as there; `connected` says what generate_TM printed;
//   * sizes are capped (FSM_MAX_*) where an int product of the reference would overflow or a table would not fit.
// Not built: write_trellis_svg, write_fsm_txt.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace grhip {

constexpr int FSM_MAX_S = 2048;             // TMl / TMi hold S * S ints
constexpr int FSM_MAX_I = 1 << 21;          // the decoder packs an input symbol beside a state
constexpr int FSM_MAX_O = 1 << 24;
constexpr long long FSM_MAX_IS = 1 << 22;   // NS / OS hold I * S ints

struct Fsm {
    int I = 0, S = 0, O = 0;
    std::vector<int> NS, OS;
    std::vector<std::vector<int> > PS, PI;
    std::vector<int> TMi, TMl;
    bool connected = true;
};

// ---- base.cc ---------------------------------------------------------------------------------------------------------
inline bool fsm_dec2base(unsigned int num, int base, std::vector<int> &s)               // base.cc:29-43
{
    int l = (int)s.size();
    unsigned int n = num;
    for (int i = 0; i < l; i++) {
        s[l - i - 1] = n % base;   // MSB first
        n /= base;
    }
    return n == 0;
}

inline unsigned int fsm_base2dec(const std::vector<int> &s, int base)                   // base.cc:46-53
{
    int l = (int)s.size();
    unsigned int num = 0;
    for (int i = 0; i < l; i++) num = num * base + s[i];
    return num;
}

inline bool fsm_dec2bases(unsigned int num, const std::vector<int> &bases, std::vector<int> &s)    // base.cc:56-70
{
    int l = (int)s.size();
    unsigned int n = num;
    for (int i = 0; i < l; i++) {
        s[l - i - 1] = n % bases[l - i - 1];
        n /= bases[l - i - 1];
    }
    return n == 0;
}

inline unsigned int fsm_bases2dec(const std::vector<int> &s, const std::vector<int> &bases)         // base.cc:74-81
{
    int l = (int)s.size();
    unsigned int num = 0;
    for (int i = 0; i < l; i++) num = num * bases[i] + s[i];
    return num;
}

// ---- the tables every constructor ends with --------------------------------------------------------------------------
inline bool fsm_sizes_ok(long long I, long long S, long long O)
{
    return I >= 1 && S >= 1 && O >= 1 && I <= FSM_MAX_I && S <= FSM_MAX_S && O <= FSM_MAX_O && I * S <= FSM_MAX_IS;
}

// fsm.cc:377-395: PS[i] and PI[i] list the (state, input) pairs that lead to i, in ascending (state, input) order
inline void fsm_generate_PS_PI(Fsm &f)
{
    f.PS.assign(f.S, std::vector<int>());
    f.PI.assign(f.S, std::vector<int>());
    for (int ii = 0; ii < f.S; ii++)
        for (int jj = 0; jj < f.I; jj++) {
            const int i = f.NS[(size_t)ii * f.I + jj];
            f.PS[i].push_back(ii);
            f.PI[i].push_back(jj);
        }
}

inline bool fsm_find_es(Fsm &f, int es)                                                 // fsm.cc:430-452
{
    const int d_S = f.S, d_I = f.I;
    bool done = true;
    for (int s = 0; s < d_S; s++) {
        if (f.TMl[(size_t)s * d_S + es] < d_S) continue;
        int minl = d_S;
        int mini = -1;
        for (int i = 0; i < d_I; i++) {
            if (1 + f.TMl[(size_t)f.NS[(size_t)s * d_I + i] * d_S + es] < minl) {
                minl = 1 + f.TMl[(size_t)f.NS[(size_t)s * d_I + i] * d_S + es];
                mini = i;
            }
        }
        if (mini != -1) {
            f.TMl[(size_t)s * d_S + es] = minl;
            f.TMi[(size_t)s * d_S + es] = mini;
        } else
            done = false;
    }
    return done;
}

inline void fsm_generate_TM(Fsm &f)                                                     // fsm.cc:401-426
{
    const int d_S = f.S;
    f.TMi.assign((size_t)d_S * d_S, -1);      // no meaning
    f.TMl.assign((size_t)d_S * d_S, d_S);     // infinity: you need at most S-1 steps
    for (int i = 0; i < d_S; i++) f.TMl[(size_t)i * d_S + i] = 0;
    f.connected = true;
    for (int s = 0; s < d_S; s++) {
        bool done = false;
        int attempts = 0;
        while (done == false && attempts < d_S - 1) {
            done = fsm_find_es(f, s);
            attempts++;
        }
        if (done == false && d_S > 1) f.connected = false;      // :420-424 prints and goes on
    }
}

// validate I, S, O, NS, OS and build PS, PI, TMl, TMi; false where the tables are refused
inline bool fsm_finish(Fsm &f)
{
    if (!fsm_sizes_ok(f.I, f.S, f.O)) return false;
    const size_t n = (size_t)f.I * f.S;
    if (f.NS.size() != n || f.OS.size() != n) return false;
    for (size_t i = 0; i < n; i++)
        if (f.NS[i] < 0 || f.NS[i] >= f.S || f.OS[i] < 0 || f.OS[i] >= f.O) return false;
    fsm_generate_PS_PI(f);
    fsm_generate_TM(f);
    return true;
}

// ---- the constructors ------------------------------------------------------------------------------------------------
inline bool fsm_from_tables(int I, int S, int O, const std::vector<int> &NS, const std::vector<int> &OS, Fsm &out)    // fsm.cc:60-70
{
    Fsm f;
    f.I = I; f.S = S; f.O = O; f.NS = NS; f.OS = OS;
    if (!fsm_finish(f)) return false;
    out = std::move(f);
    return true;
}

// the text of an .fsm file (fsm.cc:82-117): "I S O", then S * I next states, then S * I outputs; what follows is comment
inline bool fsm_from_text(const char *text, Fsm &out)
{
    if (!text) return false;
    const char *p = text;
    auto next = [&](int &v) {
        char *end = nullptr;
        const long x = std::strtol(p, &end, 10);                // skips white space, as %d does
        if (end == p || x < -2147483647L - 1 || x > 2147483647L) return false;
        v = (int)x;
        p = end;
        return true;
    };
    Fsm f;
    if (!next(f.I) || !next(f.S) || !next(f.O) || !fsm_sizes_ok(f.I, f.S, f.O)) return false;
    const size_t n = (size_t)f.I * f.S;
    f.NS.resize(n);
    f.OS.resize(n);
    for (size_t i = 0; i < n; i++)
        if (!next(f.NS[i])) return false;
    for (size_t i = 0; i < n; i++)
        if (!next(f.OS[i])) return false;
    if (!fsm_finish(f)) return false;
    out = std::move(f);
    return true;
}

inline bool fsm_from_file(const char *name, Fsm &out)
{
    if (!name) return false;
    FILE *fp = std::fopen(name, "r");
    if (!fp) return false;
    std::string text;
    char buf[4096];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof(buf), fp)) > 0) {
        text.append(buf, got);
        if (text.size() > ((size_t)1 << 30)) break;
    }
    std::fclose(fp);
    return fsm_from_text(text.c_str(), out);
}

// the (n, k) binary convolutional code with generator matrix G, k * n entries (fsm.cc:125-224)
inline bool fsm_from_generator(int k, int n, const std::vector<int> &G, Fsm &out)
{
    if (k < 1 || n < 1 || k > 21 || n > 24 || G.size() != (size_t)k * n) return false;
    for (int g : G)
        if (g < 0) return false;
    // calculate maximum memory requirements for each input stream
    std::vector<int> max_mem_x(k, -1);
    int max_mem = -1;
    for (int i = 0; i < k; i++) {
        for (int j = 0; j < n; j++) {
            int mem = -1;
            if (G[i * n + j] != 0) mem = (int)(log(double(G[i * n + j])) / log(2.0));
            if (mem > max_mem_x[i]) max_mem_x[i] = mem;
            if (mem > max_mem) max_mem = mem;
        }
    }
    // calculate total memory requirements to set S; an all-zero row would shift by -1 in the reference
    int sum_max_mem = 0;
    for (int i = 0; i < k; i++) {
        if (max_mem_x[i] < 0) return false;
        sum_max_mem += max_mem_x[i];
    }
    if (sum_max_mem > 11) return false;             // S <= FSM_MAX_S
    Fsm f;
    f.I = 1 << k;
    f.S = 1 << sum_max_mem;
    f.O = 1 << n;
    if (!fsm_sizes_ok(f.I, f.S, f.O)) return false;
    const int d_I = f.I, d_S = f.S;

    // binary representation of the G matrix
    std::vector<std::vector<int> > Gb(k * n);
    for (int j = 0; j < k * n; j++) {
        Gb[j].resize(max_mem + 1);
        fsm_dec2base(G[j], 2, Gb[j]);
    }
    // alphabet size of each shift register
    std::vector<int> bases_x(k);
    for (int j = 0; j < k; j++) bases_x[j] = 1 << max_mem_x[j];

    f.NS.resize((size_t)d_I * d_S);
    f.OS.resize((size_t)d_I * d_S);

    std::vector<int> sx(k);
    std::vector<int> nsx(k);
    std::vector<int> tx(k);
    std::vector<std::vector<int> > tb(k);
    for (int j = 0; j < k; j++) tb[j].resize(max_mem + 1);
    std::vector<int> inb(k);
    std::vector<int> outb(n);

    for (int s = 0; s < d_S; s++) {
        fsm_dec2bases(s, bases_x, sx);     // split s into k values, each representing one of the k shift registers
        for (int i = 0; i < d_I; i++) {
            fsm_dec2base(i, 2, inb);       // input in binary
            // evaluate next state
            for (int j = 0; j < k; j++) nsx[j] = (inb[j] * bases_x[j] + sx[j]) / 2;     // MSB first
            f.NS[(size_t)s * d_I + i] = (int)fsm_bases2dec(nsx, bases_x);
            // evaluate transitions
            for (int j = 0; j < k; j++) tx[j] = inb[j] * bases_x[j] + sx[j];
            for (int j = 0; j < k; j++) fsm_dec2base(tx[j], 2, tb[j]);
            // evaluate outputs
            for (int nn = 0; nn < n; nn++) {
                outb[nn] = 0;
                for (int j = 0; j < k; j++)
                    for (int m = 0; m < max_mem + 1; m++)
                        outb[nn] = (outb[nn] + Gb[j * n + nn][m] * tb[j][m]) % 2;       // 1+D is 110, not 011
            }
            f.OS[(size_t)s * d_I + i] = (int)fsm_base2dec(outb, 2);
        }
    }
    if (!fsm_finish(f)) return false;
    out = std::move(f);
    return true;
}

// (int)(pow(base, e) + 0.5) of the reference, or 0 where it would pass `cap`
inline int fsm_ipow(int base, int e, long long cap)
{
    const double v = pow(1.0 * base, 1.0 * e);
    if (!(v >= 0.5) || v > (double)cap) return 0;
    return (int)(v + 0.5);
}

// the ISI of a channel of length ch_length under a modulation of size mod_size (fsm.cc:234-253)
inline bool fsm_from_isi(int mod_size, int ch_length, Fsm &out)
{
    if (mod_size < 1 || ch_length < 1 || ch_length > 64) return false;
    Fsm f;
    f.I = mod_size;
    f.S = fsm_ipow(f.I, ch_length - 1, FSM_MAX_S);
    if (f.S < 1 || !fsm_sizes_ok(f.I, f.S, (long long)f.S * f.I)) return false;
    f.O = f.S * f.I;
    const int d_I = f.I, d_S = f.S;
    f.NS.resize((size_t)d_I * d_S);
    f.OS.resize((size_t)d_I * d_S);
    for (int s = 0; s < d_S; s++) {
        for (int i = 0; i < d_I; i++) {
            int t = i * d_S + s;
            f.NS[(size_t)s * d_I + i] = t / d_I;
            f.OS[(size_t)s * d_I + i] = t;
        }
    }
    if (!fsm_finish(f)) return false;
    out = std::move(f);
    return true;
}

// the trellis of a CPM with h = K / P, alphabet size M and a frequency pulse of L symbols (fsm.cc:267-292)
inline bool fsm_from_cpm(int P, int M, int L, Fsm &out)
{
    if (P < 1 || M < 1 || L < 1 || L > 64 || P > FSM_MAX_S) return false;
    const int ml1 = fsm_ipow(M, L - 1, FSM_MAX_S), ml = fsm_ipow(M, L, FSM_MAX_O);
    if (ml1 < 1 || ml < 1) return false;
    if (!fsm_sizes_ok(M, (long long)ml1 * P, (long long)ml * P)) return false;
    Fsm f;
    f.I = M;
    f.S = ml1 * P;
    f.O = ml * P;
    const int d_I = f.I, d_S = f.S;
    f.NS.resize((size_t)d_I * d_S);
    f.OS.resize((size_t)d_I * d_S);
    int nv;
    for (int s = 0; s < d_S; s++) {
        for (int i = 0; i < d_I; i++) {
            int s1 = s / P;
            int v = s % P;
            int ns1 = (i * ml1 + s1) / M;
            if (L == 1)
                nv = (i + v) % P;
            else
                nv = (s1 % M + v) % P;
            f.NS[(size_t)s * d_I + i] = ns1 * P + nv;
            f.OS[(size_t)s * d_I + i] = i * d_S + s;
        }
    }
    if (!fsm_finish(f)) return false;
    out = std::move(f);
    return true;
}

// the joint trellis of FSM1 and FSM2 (fsm.cc:307-329)
inline bool fsm_from_joint(const Fsm &FSM1, const Fsm &FSM2, Fsm &out)
{
    if (!fsm_sizes_ok((long long)FSM1.I * FSM2.I, (long long)FSM1.S * FSM2.S, (long long)FSM1.O * FSM2.O)) return false;
    Fsm f;
    f.I = FSM1.I * FSM2.I;
    f.S = FSM1.S * FSM2.S;
    f.O = FSM1.O * FSM2.O;
    const int d_I = f.I, d_S = f.S;
    f.NS.resize((size_t)d_I * d_S);
    f.OS.resize((size_t)d_I * d_S);
    for (int s = 0; s < d_S; s++) {
        for (int i = 0; i < d_I; i++) {
            int s1 = s / FSM2.S;
            int s2 = s % FSM2.S;
            int i1 = i / FSM2.I;
            int i2 = i % FSM2.I;
            f.NS[(size_t)s * d_I + i] = FSM1.NS[(size_t)s1 * FSM1.I + i1] * FSM2.S + FSM2.NS[(size_t)s2 * FSM2.I + i2];
            f.OS[(size_t)s * d_I + i] = FSM1.OS[(size_t)s1 * FSM1.I + i1] * FSM2.O + FSM2.OS[(size_t)s2 * FSM2.I + i2];
        }
    }
    if (!fsm_finish(f)) return false;
    out = std::move(f);
    return true;
}

// n stages through FSM, the radix-n FSM (fsm.cc:338-364)
inline bool fsm_from_radix(const Fsm &FSM, int n, Fsm &out)
{
    if (n < 1 || n > 64 || !fsm_sizes_ok(FSM.I, FSM.S, FSM.O)) return false;
    Fsm f;
    f.I = fsm_ipow(FSM.I, n, FSM_MAX_I);
    f.S = FSM.S;
    f.O = fsm_ipow(FSM.O, n, FSM_MAX_O);
    if (!fsm_sizes_ok(f.I, f.S, f.O)) return false;
    const int d_I = f.I, d_S = f.S;
    f.NS.resize((size_t)d_I * d_S);
    f.OS.resize((size_t)d_I * d_S);
    std::vector<int> ii(n);
    std::vector<int> oo(n);
    for (int s = 0; s < d_S; s++) {
        for (int i = 0; i < d_I; i++) {
            fsm_dec2base(i, FSM.I, ii);
            int ns = s;
            for (int k = 0; k < n; k++) {
                oo[k] = FSM.OS[(size_t)ns * FSM.I + ii[k]];
                ns = FSM.NS[(size_t)ns * FSM.I + ii[k]];
            }
            f.NS[(size_t)s * d_I + i] = ns;
            f.OS[(size_t)s * d_I + i] = (int)fsm_base2dec(oo, FSM.O);
        }
    }
    if (!fsm_finish(f)) return false;
    out = std::move(f);
    return true;
}

}  // namespace grhip
