// ModemDigital.h -- the reference's digital lab (src/modules/modem/ModemDigital.{h,cpp}, src/modules/modem/digital/*.cpp, built there with
// ENABLE_DIGITAL_LAB) over the HIP library.  As for the analog modems, the objects are host-side DESCRIPTORS: name / type, settings, rates and the
// csdr_digital_params of the bank slot; the decisions run on the device (csdr_bank_execute).  What the reference keeps in the modem
// object and the application reads back -- the lock (ModemDigital.cpp:43-53) and the console output (ModemDigitalOutput) -- stays here:
// SDRPostThread::finishDemod sets the lock from the block's csdr_digital_result and hands FSK's text to the output.
// Registration is opt-in like the reference's build switch: Modem::registerDigitalLab(), Modem::registerDigitalGMSK() for GMSK, and
// Modem::registerDigitalTables(source) for APSK, SQAM and ST (V.29), whose points are liquid's own tables: the application, which has liquid
// linked, supplies them through a ConstellationSource, and the device decides with them as caller data.
#pragma once
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "Modem.h"

class ModemKitDigital : public ModemKit {                    // ModemDigital.h:9-13
public:
    ModemKitDigital() = default;
};

class ModemDigitalOutput {                                   // ModemDigital.h:15-27: where a digital modem writes its console text
public:
    ModemDigitalOutput() = default;
    virtual ~ModemDigitalOutput() = default;
    virtual void write(std::string outp) = 0;
    virtual void write(char outc) = 0;
    virtual void Show() = 0;
    virtual void Hide() = 0;
    virtual void Close() = 0;
};

class ModemDigital : public Modem {                          // ModemDigital.h:29-60
public:
    ModemDigital() = default;
    std::string getType() override { return "digital"; }
    int checkSampleRate(long long sampleRate, int /* audioSampleRate */) override {    // ModemDigital.cpp:21-26
        return sampleRate < MIN_BANDWIDTH ? MIN_BANDWIDTH : (int)sampleRate;
    }
    ModemKit *buildKit(long long sampleRate, int audioSampleRate) override {          // ModemDigital.cpp:28-35
        ModemKitDigital *k = new ModemKitDigital;
        k->sampleRate = sampleRate; k->audioSampleRate = audioSampleRate;
        return k;
    }
    void disposeKit(ModemKit *kit) override { delete kit; }
    void setDemodulatorLock(bool demod_lock_in) { currentDemodLock.store(demod_lock_in); }
    int getDemodulatorLock() { return currentDemodLock.load(); }
    void setOutput(ModemDigitalOutput *modemDigitalOutput) { std::lock_guard<std::mutex> g(outMu_); digitalOut = modemDigitalOutput; }
    ModemDigitalOutput *getOutput() { std::lock_guard<std::mutex> g(outMu_); return digitalOut; }
    // digitalFinish (ModemDigital.cpp:65-76): the block's console text to the output, when there is any and an output is set
    void digitalFinish(const std::string &text) {
        std::lock_guard<std::mutex> g(outMu_);
        if (digitalOut && !text.empty()) digitalOut->write(text);
    }
    // the decisions run on the device: nothing may route a block through the host entry
    void demodulate(ModemKit *, ModemIQData *, AudioThreadInput *) override {
        throw std::logic_error("ModemDigital::demodulate: this modem's decisions run on the device (csdr_bank_execute)");
    }
    int csdrModemId() override { return CSDR_MODEM_DIGITAL; }
    // the slot's settings (csdr_bank_configure_digital_slot)
    virtual csdr_digital_params csdrDigitalParams() = 0;
    // the constellation the device should decide with now (writeSetting("cons") needs no rebuild: csdr_bank_set_digital_cons); 0 = none
    virtual int csdrDigitalCons() { return 0; }

protected:
    std::atomic_bool currentDemodLock{false};

private:
    std::mutex outMu_;
    ModemDigitalOutput *digitalOut = nullptr;
};

// ModemPSK / ModemDPSK / ModemASK / ModemQAM: the "cons" setting (ModemPSK.cpp:39-94 and alike); a write switches the constellation without a rebuild
template <int KIND>
class ModemDigitalCons : public ModemDigital {
public:
    static ModemBase *factory() { return new ModemDigitalCons<KIND>(); }
    std::string getName() override {
        switch (KIND) { case CSDR_DIGITAL_PSK: return "PSK"; case CSDR_DIGITAL_DPSK: return "DPSK"; case CSDR_DIGITAL_ASK: return "ASK"; }
        return "QAM";
    }
    ModemArgInfoList getSettings() override {
        ModemArgInfo a;
        a.key = "cons"; a.name = "Constellation"; a.description = "Modem Constellation Pattern"; a.value = std::to_string(cons_.load());
        for (int c = KIND == CSDR_DIGITAL_QAM ? 4 : 2; c <= 256; c *= 2) a.options.push_back(std::to_string(c));
        return ModemArgInfoList{a};
    }
    void writeSetting(std::string setting, std::string value) override {
        if (setting != "cons") return;
        const int c = std::stoi(value);
        // updateDemodulatorCons: a value outside the options leaves the object in use (its switch has no default); cons records it anyway
        bool known = false;
        for (int v = KIND == CSDR_DIGITAL_QAM ? 4 : 2; v <= 256; v *= 2) known = known || v == c;
        shownCons_.store(c);
        if (known) cons_.store(c);
    }
    std::string readSetting(std::string setting) override { return setting == "cons" ? std::to_string(shownCons_.load()) : ""; }
    csdr_digital_params csdrDigitalParams() override { csdr_digital_params p{}; p.kind = KIND; p.cons = cons_.load(); return p; }
    int csdrDigitalCons() override { return cons_.load(); }

private:
    std::atomic<int> cons_{KIND == CSDR_DIGITAL_QAM ? 4 : 2}, shownCons_{KIND == CSDR_DIGITAL_QAM ? 4 : 2};
};

// ModemBPSK / ModemQPSK / ModemOOK: no settings
template <int KIND>
class ModemDigitalFixed : public ModemDigital {
public:
    static ModemBase *factory() { return new ModemDigitalFixed<KIND>(); }
    std::string getName() override { return KIND == CSDR_DIGITAL_BPSK ? "BPSK" : (KIND == CSDR_DIGITAL_QPSK ? "QPSK" : "OOK"); }
    csdr_digital_params csdrDigitalParams() override { csdr_digital_params p{}; p.kind = KIND; return p; }
};

typedef ModemDigitalCons<CSDR_DIGITAL_PSK> ModemPSK;
typedef ModemDigitalCons<CSDR_DIGITAL_DPSK> ModemDPSK;
typedef ModemDigitalCons<CSDR_DIGITAL_ASK> ModemASK;
typedef ModemDigitalCons<CSDR_DIGITAL_QAM> ModemQAM;
typedef ModemDigitalFixed<CSDR_DIGITAL_BPSK> ModemBPSK;
typedef ModemDigitalFixed<CSDR_DIGITAL_QPSK> ModemQPSK;
typedef ModemDigitalFixed<CSDR_DIGITAL_OOK> ModemOOK;

// ModemFSK (ModemFSK.cpp): bps / sps / bw, each write asks for a rebuild; the symbols go to the output as lowercase hex
class ModemFSK : public ModemDigital {
public:
    static ModemBase *factory() { return new ModemFSK(); }
    std::string getName() override { return "FSK"; }
    int getDefaultSampleRate() override { return 19200; }
    int checkSampleRate(long long sampleRate, int /* audioSampleRate */) override {    // ModemFSK.cpp:19-28
        const double minSps = std::pow(2.0, bps_.load());
        const double nextSps = double(sampleRate) / double(sps_.load());
        return nextSps < minSps ? 2 * bps_.load() * sps_.load() : (int)sampleRate;
    }
    ModemArgInfoList getSettings() override {                                          // ModemFSK.cpp:34-76
        ModemArgInfoList args;
        ModemArgInfo b;
        b.key = "bps"; b.name = "Bits/symbol"; b.value = std::to_string(bps_.load()); b.description = "Modem bits-per-symbol"; b.units = "bits";
        b.options = {"1", "2", "4", "8", "16"};
        args.push_back(b);
        ModemArgInfo s;
        s.key = "sps"; s.name = "Symbols/second"; s.value = std::to_string(sps_.load()); s.description = "Modem symbols-per-second";
        args.push_back(s);
        ModemArgInfo w;
        w.key = "bw"; w.name = "Signal bandwidth"; w.value = std::to_string(bw_.load()); w.description = "Total signal bandwidth";
        args.push_back(w);
        return args;
    }
    void writeSetting(std::string setting, std::string value) override {               // ModemFSK.cpp:78-90
        if (setting == "bps") { bps_.store(std::stoi(value)); rebuildKit(); }
        else if (setting == "sps") { sps_.store(std::stoi(value)); rebuildKit(); }
        else if (setting == "bw") { bw_.store(std::stof(value)); rebuildKit(); }
    }
    std::string readSetting(std::string setting) override {
        if (setting == "bps") return std::to_string(bps_.load());
        if (setting == "sps") return std::to_string(sps_.load());
        if (setting == "bw") return std::to_string(bw_.load());
        return "";
    }
    csdr_digital_params csdrDigitalParams() override {
        csdr_digital_params p{};
        p.kind = CSDR_DIGITAL_FSK; p.bps = bps_.load(); p.sps = sps_.load(); p.bw = bw_.load();
        return p;
    }
    // outStream << std::hex << symbol (ModemFSK.cpp:12, :137)
    static std::string hexText(const uint32_t *sym, int n) {
        std::string s;
        char buf[16];
        for (int i = 0; i < n; ++i) { snprintf(buf, sizeof buf, "%x", sym[i]); s += buf; }
        return s;
    }

private:
    std::atomic<int> bps_{1}, sps_{9600};                                                 // ModemFSK.cpp:7-12
    std::atomic<float> bw_{0.45f};
};

// ModemGMSK (ModemGMSK.cpp): fdelay / sps (samples per symbol) / ebf, each write asks for a rebuild (a fresh gmskdem and an empty inputBuffer);
// the symbols go to the output as hex digits (0 / 1), the lock is never updated
class ModemGMSK : public ModemDigital {
public:
    static ModemBase *factory() { return new ModemGMSK(); }
    std::string getName() override { return "GMSK"; }
    int getDefaultSampleRate() override { return 19200; }                               // ModemGMSK.cpp:31-33
    ModemArgInfoList getSettings() override {                                          // ModemGMSK.cpp:35-68
        ModemArgInfoList args;
        ModemArgInfo f;
        f.key = "fdelay"; f.name = "Filter delay"; f.value = std::to_string(fdelay_.load()); f.description = "Filter delay in samples";
        f.type = ModemArgInfo::Type::INT; f.units = "samples"; f.range = ModemRange(1, 128);
        args.push_back(f);
        ModemArgInfo s;
        s.key = "sps"; s.name = "Samples / symbol"; s.value = std::to_string(sps_.load()); s.description = "Modem samples-per-symbol";
        s.type = ModemArgInfo::Type::INT; s.units = "samples/symbol"; s.range = ModemRange(2, 512);
        args.push_back(s);
        ModemArgInfo e;
        e.key = "ebf"; e.name = "Excess bandwidth"; e.value = std::to_string(ebf_.load()); e.description = "Modem excess bandwidth factor";
        e.type = ModemArgInfo::Type::FLOAT; e.range = ModemRange(0.1, 0.49);
        args.push_back(e);
        return args;
    }
    void writeSetting(std::string setting, std::string value) override {               // ModemGMSK.cpp:70-81
        if (setting == "fdelay") { fdelay_.store(std::stoi(value)); rebuildKit(); }
        else if (setting == "sps") { sps_.store(std::stoi(value)); rebuildKit(); }
        else if (setting == "ebf") { ebf_.store(std::stof(value)); rebuildKit(); }
    }
    std::string readSetting(std::string setting) override {
        if (setting == "fdelay") return std::to_string(fdelay_.load());
        if (setting == "sps") return std::to_string(sps_.load());
        if (setting == "ebf") return std::to_string(ebf_.load());
        return "";
    }
    csdr_digital_params csdrDigitalParams() override {
        csdr_digital_params p{};
        p.kind = CSDR_DIGITAL_GMSK; p.sps = sps_.load(); p.fdelay = fdelay_.load(); p.bw = ebf_.load();
        return p;
    }

private:
    std::atomic<int> sps_{4}, fdelay_{3};                                                  // ModemGMSK.cpp:7-10
    std::atomic<float> ebf_{0.3f};
};

// ---- ModemAPSK / ModemSQAM / ModemST: constellations that are liquid's own tables.  The application implements a ConstellationSource with its
// liquid -- (modem name, cons) -> the cons points modemcf_modulate returns for the symbols 0 .. cons - 1, interleaved complex; false: it has none --
// and Modem::registerDigitalTables asks it for every table of every name ONCE, as the reference's constructors create every modemcf object up
// front (ModemAPSK.cpp:6-15).  APSK tables go through csdr_design_rings, SQAM decides nearest-point behind its quadrant fold, ST nearest-point.
typedef std::function<bool(const std::string &name, int cons, std::vector<float> &points)> ConstellationSource;

enum { CSDR_HOST_TABLE_APSK = 0, CSDR_HOST_TABLE_SQAM = 1, CSDR_HOST_TABLE_ST = 2 };

class ModemDigitalTableBase : public ModemDigital {
public:
    // the slot's tables (csdr_bank_configure_table_slot), the default constellation first; they live as long as the registry
    virtual const std::vector<csdr_constellation> &csdrTables() = 0;
    csdr_digital_params csdrDigitalParams() override { csdr_digital_params p{}; p.kind = CSDR_DIGITAL_TABLE; p.cons = csdrDigitalCons(); return p; }
};

template <int WHICH>
class ModemDigitalTable : public ModemDigitalTableBase {
public:
    static ModemBase *factory() { return new ModemDigitalTable<WHICH>(); }
    static const char *modemName() { return WHICH == CSDR_HOST_TABLE_APSK ? "APSK" : (WHICH == CSDR_HOST_TABLE_SQAM ? "SQAM" : "ST"); }
    // the "cons" options (ModemAPSK.cpp:44-51, ModemSQAM.cpp:36-37); ST has no setting: its one table is V.29's 16 points
    static std::vector<int> consOptions() {
        if (WHICH == CSDR_HOST_TABLE_APSK) return {4, 8, 16, 32, 64, 128, 256};
        if (WHICH == CSDR_HOST_TABLE_SQAM) return {32, 128};
        return {16};
    }
    static std::vector<csdr_constellation> &tables() { static std::vector<csdr_constellation> t; return t; }
    // every table of this modem from the source; false (and nothing kept) when one is missing or is not what its rule needs
    static bool loadTables(const ConstellationSource &source) {
        std::vector<csdr_constellation> t;
        for (int cons : consOptions()) {
            std::vector<float> pts;
            if (!source || !source(modemName(), cons, pts) || pts.size() != (size_t)2 * cons) return false;
            csdr_constellation c;
            if (WHICH == CSDR_HOST_TABLE_APSK) { if (csdr_design_rings(pts.data(), cons, &c) != CSDR_OK) return false; }
            else {
                std::memset(&c, 0, sizeof c);
                c.rule = WHICH == CSDR_HOST_TABLE_SQAM ? CSDR_TABLE_QUADRANT : CSDR_TABLE_NEAREST; c.n_points = cons;
                std::memcpy(c.points, pts.data(), pts.size() * sizeof(float));
            }
            c.sensitivity = 0.005f;                                  // updateDemodulatorLock(mod, 0.005f): ModemAPSK.cpp:116, ModemSQAM.cpp:78, ModemST.cpp:30
            t.push_back(c);
        }
        tables() = std::move(t);
        return true;
    }
    std::string getName() override { return modemName(); }
    ModemArgInfoList getSettings() override {
        if (WHICH == CSDR_HOST_TABLE_ST) return ModemArgInfoList();
        ModemArgInfo a;
        a.key = "cons"; a.name = "Constellation"; a.description = "Modem Constellation Pattern"; a.value = std::to_string(shownCons_.load());
        for (int c : consOptions()) a.options.push_back(std::to_string(c));
        return ModemArgInfoList{a};
    }
    void writeSetting(std::string setting, std::string value) override {        // updateDemodulatorCons: a pointer move, no rebuild
        if (WHICH == CSDR_HOST_TABLE_ST || setting != "cons") return;
        const int c = std::stoi(value);
        shownCons_.store(c);
        for (int v : consOptions()) if (v == c) cons_.store(c);                  // (a value outside the options leaves the object in use)
    }
    std::string readSetting(std::string setting) override { return (WHICH != CSDR_HOST_TABLE_ST && setting == "cons") ? std::to_string(shownCons_.load()) : ""; }
    int csdrDigitalCons() override { return cons_.load(); }
    const std::vector<csdr_constellation> &csdrTables() override { return tables(); }

private:
    std::atomic<int> cons_{consOptions().front()}, shownCons_{consOptions().front()};
};

typedef ModemDigitalTable<CSDR_HOST_TABLE_APSK> ModemAPSK;
typedef ModemDigitalTable<CSDR_HOST_TABLE_SQAM> ModemSQAM;
typedef ModemDigitalTable<CSDR_HOST_TABLE_ST> ModemST;

// APSK, SQAM and ST (CubicSDR.cpp:315-328 registers them beside the others), opt-in and only with a source of their points: a name whose tables the
// source cannot supply is not registered.  Returns the number of names registered by this call; names registered earlier keep their tables.
inline int Modem::registerDigitalTables(const ConstellationSource &source) {
    registerBuiltins();
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    int n = 0;
    if (ModemAPSK::tables().empty() && ModemAPSK::loadTables(source)) { addModemFactory(ModemAPSK::factory, "APSK", 200000); ++n; }
    if (ModemSQAM::tables().empty() && ModemSQAM::loadTables(source)) { addModemFactory(ModemSQAM::factory, "SQAM", 200000); ++n; }
    if (ModemST::tables().empty() && ModemST::loadTables(source)) { addModemFactory(ModemST::factory, "ST", 200000); ++n; }
    return n;
}

// GMSK is registered on its own (CubicSDR.cpp:321 registers it beside the others): registerDigitalLab's list stays the one it was
inline void Modem::registerDigitalGMSK() {
    registerBuiltins();
    static std::once_flag once;
    std::call_once(once, [] { addModemFactory(ModemGMSK::factory, "GMSK", 19200); });
}

inline void Modem::registerDigitalLab() {                                               // CubicSDR.cpp:315-328 (the built ones)
    registerBuiltins();
    static std::once_flag once;
    std::call_once(once, [] {
    addModemFactory(ModemASK::factory, "ASK", 200000);
    addModemFactory(ModemBPSK::factory, "BPSK", 200000);
    addModemFactory(ModemDPSK::factory, "DPSK", 200000);
    addModemFactory(ModemFSK::factory, "FSK", 19200);
    addModemFactory(ModemOOK::factory, "OOK", 200000);
    addModemFactory(ModemPSK::factory, "PSK", 200000);
    addModemFactory(ModemQAM::factory, "QAM", 200000);
    addModemFactory(ModemQPSK::factory, "QPSK", 200000);
    });
}
