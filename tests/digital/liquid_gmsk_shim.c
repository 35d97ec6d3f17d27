/*
 * liquid_gmsk_shim.c -- TEST INFRASTRUCTURE ONLY.  Compiled by tests/gmsk_oracle.py at test time and linked against the oracle's loader of
 * the reference liquid-dsp 1.5.0 binary; the product never sees it.
 *
 * SysV wrappers around the ms_abi exports of the reference's GMSK modem (ModemGMSK.cpp): gmskdem_create / _demodulate / _reset / _destroy,
 * gmskmod_create / _modulate / _destroy, and the filter designs liquid_firdes_gmsktx / _gmskrx.
 */
#include <stddef.h>
#include <stdint.h>

#define MS __attribute__((ms_abi))

int liquid_ref_load(const char *path);
void *pe_sym(const char *name);

typedef void *(MS *gmsk_create_t)(unsigned int, unsigned int, float);
typedef int (MS *gmsk_destroy_t)(void *);
typedef int (MS *gmskdem_demod_t)(void *, const float *, unsigned int *);
typedef int (MS *gmskmod_mod_t)(void *, unsigned int, float *);
typedef int (MS *firdes_gmsk_t)(unsigned int, unsigned int, float, float, float *);

static void *sym(const char *name)
{
    if (liquid_ref_load(NULL)) return 0;
    return pe_sym(name);
}

int shim_gmsk_ready(void)
{
    return sym("gmskdem_create") && sym("gmskdem_demodulate") && sym("gmskdem_reset") && sym("gmskdem_destroy") && sym("gmskmod_create") &&
           sym("gmskmod_modulate") && sym("gmskmod_destroy") && sym("liquid_firdes_gmsktx") && sym("liquid_firdes_gmskrx");
}

void *shim_gmskdem_create(unsigned int k, unsigned int m, float bt) { return ((gmsk_create_t)sym("gmskdem_create"))(k, m, bt); }
void shim_gmskdem_reset(void *q) { ((gmsk_destroy_t)sym("gmskdem_reset"))(q); }
void shim_gmskdem_destroy(void *q) { ((gmsk_destroy_t)sym("gmskdem_destroy"))(q); }

/* n_sym calls of gmskdem_demodulate, each on the k interleaved complex samples at iq + 2 k i */
void shim_gmskdem_run(void *q, const float *iq, int n_sym, int k, uint32_t *out)
{
    gmskdem_demod_t f = (gmskdem_demod_t)sym("gmskdem_demodulate");
    for (int i = 0; i < n_sym; i++) {
        unsigned int s = 0;
        f(q, iq + 2 * (size_t)i * k, &s);
        out[i] = s;
    }
}

void *shim_gmskmod_create(unsigned int k, unsigned int m, float bt) { return ((gmsk_create_t)sym("gmskmod_create"))(k, m, bt); }
void shim_gmskmod_destroy(void *q) { ((gmsk_destroy_t)sym("gmskmod_destroy"))(q); }

/* n_sym symbols through the modulator: k samples each */
void shim_gmskmod_run(void *q, const uint32_t *in, int n_sym, int k, float *out)
{
    gmskmod_mod_t f = (gmskmod_mod_t)sym("gmskmod_modulate");
    for (int i = 0; i < n_sym; i++) f(q, in[i], out + 2 * (size_t)i * k);
}

int shim_firdes_gmsktx(unsigned int k, unsigned int m, float bt, float *h) { return ((firdes_gmsk_t)sym("liquid_firdes_gmsktx"))(k, m, bt, 0.0f, h); }
int shim_firdes_gmskrx(unsigned int k, unsigned int m, float bt, float *h) { return ((firdes_gmsk_t)sym("liquid_firdes_gmskrx"))(k, m, bt, 0.0f, h); }
