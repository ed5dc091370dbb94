// capi_genbank.cc -- C ABI, GenBank input and accuracy evaluation (host only): augx_input_type, augx_genbank_*, augx_eval_*.
// (augx_genbank_report lives in driver.cc, next to the writer of the predictions it shares with augx_main.)
#include <cstring>
#include <fstream>
#include <sstream>
#include "capi_internal.h"

using namespace augx;

namespace {

int mod3(int k) { return k >= 0 ? k % 3 : (k % 3 + 3) % 3; }

int copyOut(const std::string &text, char *out, int64_t cap, const char *who) {
    if ((int64_t)text.size() + 1 > cap) { setLastError(std::string(who) + ": output buffer too small"); return AUGX_E_ARG; }
    memcpy(out, text.c_str(), text.size() + 1);
    return AUGX_OK;
}

// the transcript of the evaluation from its flat form
Transcript fromFlat(const augx_transcript &a) {
    Transcript t;
    t.plus = a.strand >= 0;
    t.complete = a.complete != 0;
    t.complete5utr = a.complete_5utr != 0;
    t.complete3utr = a.complete_3utr != 0;
    t.transstart = (long)a.trans_start;
    t.transend = (long)a.trans_end;
    t.codingstart = (long)a.coding_start;
    t.codingend = (long)a.coding_end;
    if (a.gene_id) t.geneid = a.gene_id;
    if (a.transcript_id) t.id = a.transcript_id;
    for (int i = 0; i < a.n_exons; i++) {
        BioState s;
        s.begin = (long)a.exons[i].begin;
        s.end = (long)a.exons[i].end;
        (a.exons[i].kind == AUGX_EXON_UTR5 ? t.utr5exons : a.exons[i].kind == AUGX_EXON_UTR3 ? t.utr3exons : t.exons).push_back(s);
    }
    for (size_t i = 1; i < t.exons.size(); i++) {
        BioState in;
        in.begin = t.exons[i - 1].end + 1;
        in.end = t.exons[i].begin - 1;
        t.introns.push_back(in);
    }
    return t;
}

} // namespace

extern "C" {

int augx_input_type(const char *data, int64_t len) {
    if (!data || len < 0) return AUGX_INPUT_UNKNOWN;
    return (int)detectInputType(std::string(data, (size_t)len));
}

int augx_genbank_read(const char *data, int64_t len, int utr, int stop_excluded, int verbosity, augx_genbank **out) {
    if (!data || len < 0 || !out) { setLastError("augx_genbank_read: bad argument"); return AUGX_E_ARG; }
    *out = nullptr;
    augx_genbank *g = new augx_genbank();
    *out = g; // (kept on an error too: the messages up to it are the reference's)
    try {
        GbOptions go;
        go.utr = utr != 0;
        go.stopCodonExcludedFromCDS = stop_excluded != 0;
        go.verbosity = verbosity;
        std::string fatal;
        if (!readGenbank(std::string(data, (size_t)len), go, g->f, fatal)) { setLastError(fatal); return AUGX_E_CONFIG; }
        for (const GbLocus &l : g->f.loci) {
            g->exons.emplace_back();
            for (const Transcript &t : l.genes) {
                std::vector<augx_exon> ex;
                const int strand = t.plus ? 1 : -1;
                for (const BioState &s : t.utr5exons) ex.push_back({s.begin, s.end, strand, -1, AUGX_EXON_UTR5});
                for (const BioState &s : t.exons) ex.push_back({s.begin, s.end, strand, t.plus ? mod3(3 - (s.frame() - s.length())) : mod3(2 - s.frame()), AUGX_EXON_CDS});
                for (const BioState &s : t.utr3exons) ex.push_back({s.begin, s.end, strand, -1, AUGX_EXON_UTR3});
                g->exons.back().push_back(std::move(ex));
            }
        }
        return AUGX_OK;
    } catch (std::exception &e) {
        setLastError(e.what());
        return AUGX_E_CONFIG;
    }
}

int augx_genbank_read_file(const char *path, int utr, int stop_excluded, int verbosity, augx_genbank **out) {
    if (!path || !out) { setLastError("augx_genbank_read_file: bad argument"); return AUGX_E_ARG; }
    *out = nullptr;
    std::ifstream in(path);
    if (!in) { setLastError(std::string("Could not open input file \"") + path + "\"!"); return AUGX_E_CONFIG; }
    std::ostringstream ss;
    ss << in.rdbuf();
    const std::string data = ss.str();
    char wrong = ' ';
    if (detectInputType(data, &wrong) != INPUT_GENBANK) { setLastError(std::string("File format of ") + path + " not recognized as GenBank."); return AUGX_E_CONFIG; }
    return augx_genbank_read(data.data(), (int64_t)data.size(), utr, stop_excluded, verbosity, out);
}

int augx_genbank_n_loci(const augx_genbank *g) { return g ? (int)g->f.loci.size() : AUGX_E_ARG; }

const char *augx_genbank_messages(const augx_genbank *g, int stream) {
    if (!g) return "";
    return stream == 2 ? g->f.err.c_str() : g->f.out.c_str();
}

int augx_genbank_locus(const augx_genbank *g, int locus, const char **name, const char **seq, int64_t *len, int *n_transcripts) {
    if (!g || locus < 0 || locus >= (int)g->f.loci.size()) { setLastError("augx_genbank_locus: bad argument"); return AUGX_E_ARG; }
    const GbLocus &l = g->f.loci[(size_t)locus];
    if (name) *name = l.name.c_str();
    if (seq) *seq = l.seq.c_str();
    if (len) *len = l.length;
    if (n_transcripts) *n_transcripts = (int)l.genes.size();
    return AUGX_OK;
}

int augx_genbank_transcript(const augx_genbank *g, int locus, int k, augx_transcript *out) {
    if (!g || !out || locus < 0 || locus >= (int)g->f.loci.size() || k < 0 || k >= (int)g->f.loci[(size_t)locus].genes.size()) {
        setLastError("augx_genbank_transcript: bad argument");
        return AUGX_E_ARG;
    }
    const GbLocus &l = g->f.loci[(size_t)locus];
    const Transcript &t = l.genes[(size_t)k];
    const std::vector<augx_exon> &ex = g->exons[(size_t)locus][(size_t)k];
    out->gene_id = t.geneid.c_str();
    out->transcript_id = t.id.c_str();
    out->strand = t.plus ? 1 : -1;
    out->complete = t.complete ? 1 : 0;
    out->complete_left = l.completeLeft[(size_t)k];
    out->complete_right = l.completeRight[(size_t)k];
    out->complete_5utr = t.complete5utr ? 1 : 0;
    out->complete_3utr = t.complete3utr ? 1 : 0;
    out->trans_start = t.transstart;
    out->trans_end = t.transend;
    out->coding_start = t.codingstart;
    out->coding_end = t.codingend;
    out->n_exons = (int)ex.size();
    out->exons = ex.data();
    return AUGX_OK;
}

int augx_genbank_format_annotation(const augx_model *m, const augx_genbank *g, int locus, char *out, int64_t out_cap) {
    if (!m || !g || !out || locus < 0 || locus >= (int)g->f.loci.size()) { setLastError("augx_genbank_format_annotation: bad argument"); return AUGX_E_ARG; }
    try {
        OutputOptions oo;
        oo.fromModel(m->m);
        std::string text;
        printAnnotationGFF(text, g->f.loci[(size_t)locus], oo);
        return copyOut(text, out, out_cap, "augx_genbank_format_annotation");
    } catch (std::exception &e) {
        setLastError(e.what());
        return AUGX_E_CONFIG;
    }
}

void augx_genbank_destroy(augx_genbank *g) { delete g; }

augx_eval *augx_eval_create(void) { return new augx_eval(); }

int augx_eval_add(augx_eval *e, int n_pred, const augx_transcript *pred, int n_anno, const augx_transcript *anno, int strand) {
    if (!e || n_pred < 0 || n_anno < 0 || (n_pred && !pred) || (n_anno && !anno) || e->printed) { setLastError("augx_eval_add: bad argument"); return AUGX_E_ARG; }
    try {
        std::vector<Transcript> p, a;
        for (int i = 0; i < n_pred; i++) p.push_back(fromFlat(pred[i]));
        for (int i = 0; i < n_anno; i++) a.push_back(fromFlat(anno[i]));
        e->e.add(p, a, strand);
        return AUGX_OK;
    } catch (std::exception &ex) {
        setLastError(ex.what());
        return AUGX_E_NOMEM;
    }
}

int augx_eval_print(augx_eval *e, char *out, int64_t out_cap) {
    if (!e || !out || e->printed) { setLastError("augx_eval_print: bad argument"); return AUGX_E_ARG; }
    std::string text;
    e->e.finishAndPrint(text);
    e->printed = true;
    return copyOut(text, out, out_cap, "augx_eval_print");
}

void augx_eval_destroy(augx_eval *e) { delete e; }
}
