/*
 * liquid_digital_shim.c -- TEST INFRASTRUCTURE ONLY.  Compiled by tests/digital_oracle.py at test time and linked against the
 * oracle's loader of the reference liquid-dsp 1.5.0 binary; the product never sees it.
 *
 * SysV wrappers around the ms_abi exports the reference's digital modems call: modemcf_create / _modulate / _demodulate /
 * _get_demodulator_evm / _destroy and fskdem_create / _demodulate / _destroy.  A float complex passed by value travels as one
 * 64-bit integer register in that ABI, hence the uint64 packing of modemcf_demodulate's sample.
 */
#include <stdint.h>
#include <string.h>

#define MS __attribute__((ms_abi))

int liquid_ref_load(const char *path);
void *pe_sym(const char *name);

typedef void *(MS *modem_create_t)(int);
typedef int (MS *modem_demod_t)(void *, uint64_t, unsigned int *);
typedef int (MS *modem_mod_t)(void *, unsigned int, float *);
typedef float (MS *modem_evm_t)(void *);
typedef int (MS *destroy_t)(void *);
typedef void *(MS *fsk_create_t)(unsigned int, unsigned int, float);
typedef unsigned int (MS *fsk_demod_t)(void *, const float *);

static void *sym(const char *name)
{
    if (liquid_ref_load(NULL)) return 0;
    return pe_sym(name);
}

int shim_ready(void)
{
    return sym("modemcf_create") && sym("modemcf_demodulate") && sym("modemcf_modulate") && sym("modemcf_get_demodulator_evm") && sym("modemcf_destroy") &&
           sym("fskdem_create") && sym("fskdem_demodulate") && sym("fskdem_destroy");
}

void *shim_modem_create(int scheme) { return ((modem_create_t)sym("modemcf_create"))(scheme); }
void shim_modem_destroy(void *q) { ((destroy_t)sym("modemcf_destroy"))(q); }
float shim_modem_evm(void *q) { return ((modem_evm_t)sym("modemcf_get_demodulator_evm"))(q); }

/* n symbols through one object's modulator (DPSK: differential, the object keeps the phase) */
void shim_modem_modulate(void *q, const uint32_t *in, int n, float *out)
{
    modem_mod_t f = (modem_mod_t)sym("modemcf_modulate");
    for (int i = 0; i < n; i++) f(q, in[i], out + 2 * i);
}

/* n samples through one object; evm_each (may be NULL) receives the object's EVM after every sample */
void shim_modem_run(void *q, const float *iq, int n, uint32_t *out, float *evm_each)
{
    modem_demod_t f = (modem_demod_t)sym("modemcf_demodulate");
    modem_evm_t e = (modem_evm_t)sym("modemcf_get_demodulator_evm");
    for (int i = 0; i < n; i++) {
        uint64_t v;
        unsigned int s = 0;
        memcpy(&v, iq + 2 * i, 8);
        f(q, v, &s);
        out[i] = s;
        if (evm_each) evm_each[i] = e(q);
    }
}

void *shim_fsk_create(unsigned int m, unsigned int k, float bw) { return ((fsk_create_t)sym("fskdem_create"))(m, k, bw); }
void shim_fsk_destroy(void *q) { ((destroy_t)sym("fskdem_destroy"))(q); }

/* n_sym whole symbols of k samples each */
void shim_fsk_run(void *q, const float *iq, int n_sym, int k, uint32_t *out)
{
    fsk_demod_t f = (fsk_demod_t)sym("fskdem_demodulate");
    for (int i = 0; i < n_sym; i++) out[i] = f(q, iq + 2 * (size_t)i * k);
}
