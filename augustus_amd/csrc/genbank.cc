// genbank.cc -- see genbank.h
#include "genbank.h"
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <list>

namespace augx {

namespace {

const int GBMAXLINELEN = 40000; // reference include/genbank.hh:25
const int MAX_ROW_LEN = 8192;   // reference include/projectio.hh (find_line_after)

struct GbError { std::string msg; };

static inline int mod3(int k) { return k >= 0 ? k % 3 : (k % 3 + 3) % 3; }
enum { T_SINGLE = 1, T_INITIAL0 = 2, T_INTERNAL0 = 5, T_TERMINAL = 8, T_RSINGLE = 36, T_RINITIAL = 37, T_RINTERNAL0 = 38, T_RTERMINAL0 = 41 };

// the pieces of an input stream the reference's parsers rely on: formatted reads skip white space, a failed read leaves the
// stream failed and every later read fails too
struct Cursor {
    const char *p, *e;
    bool ok = true;
    Cursor(const char *b, const char *end) : p(b), e(end) {}
    void ws() { while (p < e && isspace((unsigned char)*p)) p++; }
    int peek() const { return ok && p < e ? (unsigned char)*p : -1; }
    bool get(char &c) { if (!ok || p >= e) { ok = false; return false; } c = *p++; return true; }
    void readInt(int &v) {
        if (!ok) return;
        ws();
        const char *q = p;
        if (q < e && (*q == '+' || *q == '-')) q++;
        if (q >= e || !isdigit((unsigned char)*q)) { v = 0; ok = false; return; }
        long long x = 0;
        const bool neg = *p == '-';
        for (; q < e && isdigit((unsigned char)*q); q++) x = std::min<long long>(x * 10 + (*q - '0'), INT_MAX);
        v = (int)(neg ? -x : x);
        p = q;
    }
    void readChar(char &c) { if (!ok) return; ws(); if (p >= e) { ok = false; return; } c = *p++; }
    std::string readWord() { ws(); const char *q = p; while (p < e && !isspace((unsigned char)*p)) p++; if (q == p) ok = false; return std::string(q, p); }
    // getline: the line without its '\n'
    std::string line() {
        if (!ok || p >= e) { ok = false; return std::string(); }
        const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
        std::string s(p, nl ? nl : e);
        p = nl ? nl + 1 : e;
        return s;
    }
};

// reference GBFeature (include/genbank.hh:49-70, src/genbank.cc:370-540)
struct Feature {
    std::vector<std::pair<long, long>> ranges;
    int begin = -1, end = -1;
    std::string geneid, fkey;
    bool plus = true, completeL = true, completeR = true;
    bool operator<(const Feature &o) const { return begin < o.begin || (begin == o.begin && end < o.end); }
    bool checkRange(int len) const { return begin >= 0 && end >= 0 && begin < len && end < len; }
    // whether `other` (an mRNA) extends this (a CDS): identical where this has exons, reaching at least as far at both ends
    bool matches(const Feature &other) const {
        if (!geneid.empty() && !other.geneid.empty() && geneid != other.geneid) return false;
        if (plus != other.plus) return false;
        if (ranges.empty() || other.ranges.empty()) return false;
        const size_t n = ranges.size(), m = other.ranges.size();
        size_t st = 0, ot = 0;
        while (ot < m && other.ranges[ot].second < ranges[st].second) ot++;
        if (!(ot < m && other.ranges[ot].first <= ranges[st].first &&
              (other.ranges[ot].second == ranges[st].second || (st + 1 == n && other.ranges[ot].second >= ranges[st].second))))
            return false;
        while (ot + 1 < m && st + 1 < n) {
            st++;
            ot++;
            if (!(st + 1 == n || st == 0) && !(ranges[st] == other.ranges[ot])) return false;
        }
        if (st + 1 < n) return false;
        if (!(other.ranges[ot].second >= ranges[st].second && (other.ranges[ot].first == ranges[st].first || (st == 0 && other.ranges[ot].first <= ranges[st].first))))
            return false;
        return true;
    }
};

// reference GBFeature::GBFeature(const char *): the location of the feature that begins at `text` (complement(...), join(...),
// one nested in the other, a plain range; '<' and '>' mark a partial end), the /gene= qualifier among the lines that follow
Feature parseFeature(const char *text, const char *end, std::string &err) {
    Feature f;
    Cursor s(text, end);
    f.fkey = s.readWord();
    s.ws();
    int c = s.peek();
    char ch = 0;
    if (c == 'c') { // "complement"
        f.plus = false;
        while (s.get(ch) && ch != '(' && ch != '\n') {}
    }
    c = s.peek();
    std::string tmp;
    auto tooLong = [&]() {
        err += "Genbank feature description of " + f.fkey + "  " + tmp.substr(0, 40) + " ... reaches the character limit of " + std::to_string(GBMAXLINELEN - 1) + "\n";
        throw GbError{"GBProcessor::getJoin( ):  failed!!!"};
    };
    if (c >= 0 && isalpha(c)) { // join( or another operator: its ranges, which may go over several lines
        while (s.get(ch) && ch != '(' && ch != '\n') {}
        if (ch == '\n') {
            err += "Feature key = " + f.fkey + ", c = " + ch + "\n";
            throw GbError{"GBProcessor::getJoin( ):  failed!!!"};
        }
        while (s.get(ch) && ch != ')')
            if (!isspace((unsigned char)ch)) {
                if (isdigit((unsigned char)ch) || ch == '.' || ch == ',' || ch == '<' || ch == '>') {
                    if ((int)tmp.size() >= GBMAXLINELEN) tooLong();
                    tmp += ch;
                } else { // e.g. join(complement(..),..), order(..) of operators, a reference to another entry (J00194.1:1..5)
                    err += f.fkey + " contains character " + ch + "\n";
                    throw GbError{"GBProcessor::getJoin( ):  failed!!!"};
                }
            }
        while (s.get(ch) && ch != '\n') {}
    } else if ((c >= 0 && isdigit(c)) || c == '<') {
        while (s.get(ch) && ch != ')' && ch != '\n') {
            if ((int)tmp.size() >= GBMAXLINELEN) tooLong();
            tmp += ch;
        }
        while (s.ok && ch != '\n') s.get(ch);
    } else {
        err += "Feature key = " + f.fkey + ", c = " + (char)c + "\n";
        throw GbError{"GBProcessor::getJoin( ):  failed!!!"};
    }
    // the name of the gene: the first /gene= among the qualifier lines (21 blanks) that follow
    for (bool done = false; s.ok && !done;) {
        const std::string buf = s.line().substr(0, GBMAXLINELEN - 2);
        if (strncmp(buf.c_str(), "                     ", 21) != 0) { f.geneid = ""; done = true; }
        else {
            const size_t g = buf.find("/gene=");
            if (g != std::string::npos) {
                const size_t from = std::min(buf.size(), g + 7);
                f.geneid = buf.substr(from, buf.find('"', from) == std::string::npos ? std::string::npos : buf.find('"', from) - from);
                done = true;
            }
        }
    }
    // the ranges
    Cursor j(tmp.data(), tmp.data() + tmp.size());
    std::string why;
    while (j.ok) {
        char d = 0;
        int ebegin = -1, eend = -1;
        if (j.peek() == '<') { f.completeL = false; j.get(d); }
        j.readInt(ebegin);
        j.readChar(d);
        j.readChar(d);
        if (j.peek() == '>') { f.completeR = false; j.get(d); }
        j.readInt(eend);
        j.readChar(d); // format: 'Number..Number,'
        if (ebegin < 1 || eend < 1) { why = "Wrong format for coordinates: " + tmp; break; }
        if (ebegin > eend) { why = "Feature begins after it ends: " + tmp; break; }
        f.ranges.push_back({ebegin - 1, eend - 1});
        if (f.begin == -1 || ebegin - 1 < f.begin) f.begin = ebegin - 1;
        if (f.end == -1 || eend - 1 > f.end) f.end = eend - 1;
    }
    if (!why.empty()) {
        err += "Constructing GenBank feature: " + why + "\n";
        throw GbError{"GBFeature constructor:Format error when reading genbank format."};
    }
    return f;
}

// reference Gene::addUTR: the UTR exons of gene t from the ranges of its mRNA feature
void addUTR(Transcript &t, const std::vector<std::pair<long, long>> &mrna, bool completeL, bool completeR) {
    const bool cds = !t.exons.empty();
    if (!completeL && !completeR && !cds) return; // no CDS and mRNA incomplete at both ends: cannot be used
    if (completeL && completeR && !cds) return;   // no CDS and mRNA complete at both ends: cannot be used
    long transstart = INT_MAX, transend = -1;
    auto utrExon = [](long b, long e) { BioState s; s.begin = b; s.end = e; return s; };
    for (const auto &r : mrna) {
        transstart = std::min(transstart, r.first);
        transend = std::max(transend, r.second);
        if (cds) {
            if (r.first < t.codingstart) (t.plus ? t.utr5exons : t.utr3exons).push_back(utrExon(r.first, r.second < t.codingstart ? r.second : t.codingstart - 1));
            if (r.second > t.codingend) (t.plus ? t.utr3exons : t.utr5exons).push_back(utrExon(r.first > t.codingend ? r.first : t.codingend + 1, r.second));
        } else if ((t.plus && !completeR) || (!t.plus && !completeL)) t.utr5exons.push_back(utrExon(r.first, r.second));
        else t.utr3exons.push_back(utrExon(r.first, r.second));
    }
    if (cds) {
        t.complete5utr = t.plus ? completeL : completeR;
        t.complete3utr = t.plus ? completeR : completeL;
    } else if ((t.plus && !completeR) || (!t.plus && !completeL)) { t.complete5utr = true; t.complete3utr = false; }
    else { t.complete3utr = true; t.complete5utr = false; }
    if (transstart == INT_MAX) transstart = -1;
    if (transstart > t.codingstart && t.codingstart > 0) transstart = t.codingstart;
    if (transend > 0 && transend < t.codingend) transend = t.codingend;
    t.transstart = transstart;
    t.transend = transend;
}

struct Positions { // reference GBPositions
    const char *buffer = nullptr, *bufEnd = nullptr, *seqbegin = nullptr;
    int seqlength = 0;
    std::list<Feature> CDS, mRNA;
};

// reference GBProcessor::getSequence: the letters of the lines after ORIGIN, each line after its leading number
std::string getSequence(Positions &pos, std::string &err) {
    std::string seq;
    Cursor s(pos.seqbegin, pos.bufEnd);
    {   // the ORIGIN line itself (read into a buffer of seqlength + 1 characters: a longer line fails the stream)
        const char *nl = (const char *)memchr(s.p, '\n', (size_t)(s.e - s.p));
        const long lineLen = (nl ? nl : s.e) - s.p;
        if (lineLen > pos.seqlength) s.ok = false;
        s.p = nl ? nl + 1 : s.e;
    }
    int count = 0;
    while (s.ok) {
        int i = 0;
        s.readInt(i);
        char c;
        while (s.get(c) && c != '\n')
            if (isalpha((unsigned char)c)) {
                if (count++ < pos.seqlength) seq.push_back(c);
                else {
                    char buffer[200];
                    snprintf(buffer, sizeof buffer, "Sequence was longer than the expected %d bp. Please compare the line 'source 1..X' with the actual sequence length.", pos.seqlength);
                    throw GbError{buffer};
                }
            }
    }
    if (count < pos.seqlength) {
        err += "Warning: Sequence was shorter than expected frome the source line of the Genbank entry ( expected " + std::to_string(pos.seqlength) +
               " bp). Please compare the line 'source 1..X' with the actual sequence length (" + std::to_string(count) + ").\n";
        pos.seqlength = count;
    }
    return seq;
}

// reference GBSplitter::findPositions on the text of one entry (up to and with its "//" line)
void findPositions(Positions &pos, GbFile &res) {
    Cursor s(pos.buffer, pos.bufEnd);
    while (s.ok) {
        const char *curpos = s.p;
        s.ws();
        const std::string buf = s.line();
        if ((int)buf.size() >= GBMAXLINELEN - 2)
            throw GbError{"Could not read the following line in Genbank file.\n" + buf.substr(0, GBMAXLINELEN - 2) +
                          "\nPossible reasons: line too long or file too large. Maximum line length is \n" + std::to_string(GBMAXLINELEN - 2) + ".\n"};
        if (buf.compare(0, 6, "source") == 0) {
            Cursor l(buf.data(), buf.data() + buf.size());
            int a = 0, b = 0;
            char c = 0;
            l.readWord();
            l.readInt(a); l.readChar(c); l.readChar(c); l.readInt(b);
            if (!l.ok) throw GbError{"Syntax error in source line:\n" + buf + "\nShould be of a format like:  source  1..2345"};
            if (b - a + 1 > pos.seqlength) pos.seqlength = b - a + 1;
            continue;
        }
        if (buf.compare(0, 13, "mRNA         ") == 0) {
            Feature f = parseFeature(curpos, pos.bufEnd, res.err);
            if (f.checkRange(pos.seqlength)) pos.mRNA.push_back(f);
            else res.out += "mRNA " + f.geneid + " out of range. Ignoring it.\nend= " + std::to_string(f.end) + " len= " + std::to_string(pos.seqlength) + "\n";
        }
        if (buf.compare(0, 16, "CDS             ") == 0) {
            Feature f = parseFeature(curpos, pos.bufEnd, res.err);
            if (f.checkRange(pos.seqlength)) pos.CDS.push_back(f);
            else res.out += "CDS " + f.geneid + " out of range. Ignoring it.\n";
        }
        if (buf.compare(0, 6, "ORIGIN") == 0) {
            pos.seqbegin = curpos;
            break;
        }
    }
    if (pos.seqlength == 0) throw GbError{"Sequence has 0 length. Maybe 'source' Feature missing?"};
}

// reference GBProcessor::getAnnoSequence
GbLocus getAnnoSequence(Positions &pos, const GbOptions &go, GbFile &res) {
    GbLocus L;
    // (the reference reads the sequence through a pointer it sets at the ORIGIN line only: without that line it reads through a
    //  pointer that was never set.  Refused by name.)
    if (!pos.seqbegin) throw GbError{"No 'ORIGIN' line in the entry: no sequence."};
    L.seq = getSequence(pos, res.err);
    L.length = pos.seqlength;
    {
        const char *id = nullptr;
        for (const char *q = pos.buffer; q + 5 <= pos.bufEnd; q++)
            if (memcmp(q, "LOCUS", 5) == 0) { id = q + 5; break; }
        if (!id) L.name = "unknown";
        else {
            while (id < pos.bufEnd && isspace((unsigned char)*id)) id++;
            for (int i = 0; i < 99 && id < pos.bufEnd && !isspace((unsigned char)*id); i++, id++) L.name.push_back(*id);
        }
    }
    if (pos.CDS.empty() && go.verbosity > 0) res.err += "No 'CDS' found in sequence " + L.name + "\n";
    std::vector<Transcript> allgenes;
    std::vector<std::pair<char, char>> ends; // (complete at the left, at the right) of the feature a gene was made from
    int curGeneNr = 1, lastgeneend = -1;
    pos.CDS.sort();
    pos.mRNA.sort();
    auto newGene = [&](const Feature &f) {
        Transcript g;
        g.id = "1";
        g.geneid = !f.geneid.empty() ? f.geneid : L.name + "-" + std::to_string(curGeneNr);
        g.seqname = L.name;
        g.plus = f.plus;
        g.clength = 0;
        g.codingstart = g.codingend = -1;
        return g;
    };
    // genes from the CDS features first
    for (Feature &fit : pos.CDS) {
        bool cont = true;
        if (fit.begin <= lastgeneend) {
            res.err += "CDS overlaps with other CDS (" + std::to_string(fit.begin + 1) + " <= " + std::to_string(lastgeneend + 1) + ") in sequence " + L.name + ". Ignoring this gene.\n";
            cont = false;
        }
        if (cont && go.verbosity > 0 && (!fit.completeL || !fit.completeR)) res.err += "Coding sequence incomplete in sequence " + L.name + ".\n";
        if (!cont) continue;
        Transcript g = newGene(fit);
        const size_t n = fit.ranges.size();
        for (size_t k = 0; k < n; k++) {
            std::pair<long, long> &st = fit.ranges[k]; // (the stop codon added below is seen by the match with the mRNA features, as in the reference)
            g.clength += (int)(st.second - st.first + 1);
            int type;
            if (k == 0) type = n == 1 ? (fit.plus ? T_SINGLE : T_RSINGLE) : fit.plus ? T_INITIAL0 + mod3(g.clength) : T_RTERMINAL0 + mod3(2 - g.clength);
            else if (k + 1 == n) type = fit.plus ? T_TERMINAL : T_RINITIAL;
            else type = fit.plus ? T_INTERNAL0 + mod3(g.clength) : T_RINTERNAL0 + mod3(2 - g.clength);
            if (go.stopCodonExcludedFromCDS) {
                if (type == T_SINGLE || type == T_TERMINAL) { g.clength += 3; st.second += 3; }
                if (type == T_RSINGLE || (type >= T_RTERMINAL0 && type <= T_RTERMINAL0 + 2)) { g.clength += 3; st.first -= 3; }
                if (st.first < 0 || st.second >= L.length) throw GbError{"Stop codon out of sequence bounds. Ignoring sequence."};
            }
            if (g.codingstart < 0 || g.codingstart > st.first) g.codingstart = st.first;
            if (g.codingend < st.second) g.codingend = st.second;
            if (k > 0) {
                BioState in;
                in.begin = fit.ranges[k - 1].second + 1;
                in.end = st.first - 1;
                in.type = TYPE_INTRON;
                if (in.begin > in.end) {
                    res.err += "Error: In sequence " + L.name + ": One CDS exon does not begin properly after the previous CDS exon." + std::to_string(fit.ranges[k - 1].second) +
                               " >= " + std::to_string(st.first) + "\n";
                    throw GbError{"Intron has non-positive length."};
                }
                g.introns.push_back(in);
            }
            BioState ex;
            ex.begin = st.first;
            ex.end = st.second;
            ex.type = type;
            g.exons.push_back(ex);
        }
        if (go.utr) { // the first mRNA that fits (compatible ranges, same gene name) gives the UTR; every one that fits is used up
            bool found = false;
            Feature mrna;
            for (auto it = pos.mRNA.begin(); it != pos.mRNA.end();) {
                if (fit.matches(*it)) {
                    if (!found) mrna = *it;
                    found = true;
                    it = pos.mRNA.erase(it);
                } else
                    ++it;
            }
            if (found) addUTR(g, mrna.ranges, mrna.completeL, mrna.completeR);
        }
        allgenes.push_back(g);
        ends.push_back({(char)fit.completeL, (char)fit.completeR});
        lastgeneend = fit.end;
        curGeneNr++;
    }
    if (go.utr) // incomplete genes from the mRNA features that are left
        for (const Feature &m : pos.mRNA) {
            Transcript g = newGene(m);
            addUTR(g, m.ranges, m.completeL, m.completeR);
            bool overlapsCDS = false;
            for (const Transcript &o : allgenes)
                if ((g.transstart <= o.codingstart && g.transend >= o.codingstart) || (g.transstart >= o.codingstart && g.transstart <= o.codingend)) overlapsCDS = true;
            if ((!g.utr5exons.empty() || !g.utr3exons.empty()) && !overlapsCDS) {
                allgenes.push_back(g);
                ends.push_back({(char)m.completeL, (char)m.completeR});
                curGeneNr++;
            }
        }
    if (allgenes.empty()) res.err += std::string("No correct 'CDS'") + (go.utr ? "or 'mRNA'" : "") + " found in sequence " + L.name + "\n";
    // reference sortGenePtrList: by begin, a gene before the ones already there that begin at the same base
    std::vector<size_t> order;
    for (size_t i = 0; i < allgenes.size(); i++) {
        size_t at = 0;
        while (at < order.size() && allgenes[i].geneBegin() > allgenes[order[at]].geneBegin()) at++;
        order.insert(order.begin() + (long)at, i);
    }
    for (size_t i : order) {
        L.genes.push_back(allgenes[i]);
        L.completeLeft.push_back(ends[i].first);
        L.completeRight.push_back(ends[i].second);
    }
    return L;
}

} // namespace

InputType detectInputType(const std::string &data, char *wrongChar) {
    if (wrongChar) *wrongChar = ' ';
    {   // GenBank: a line that begins with LOCUS and, after it, one that begins with ORIGIN (blanks before either do not count)
        Cursor s(data.data(), data.data() + data.size());
        s.ws();
        int found = 0;
        for (const char *key : {"LOCUS", "ORIGIN"}) {
            bool hit = false;
            do {
                s.ws();
                const bool more = s.p < s.e;
                const char *b = s.p;
                const std::string l = s.line();
                if ((int)l.size() >= MAX_ROW_LEN - 1) { s.ok = false; s.p = b + MAX_ROW_LEN - 2; } // (a longer line fails the reference's stream)
                if (strncmp(l.c_str(), key, strlen(key)) == 0) { hit = true; break; }
                if (!more) s.ok = false;
            } while (s.ok);
            if (!hit) break;
            found++;
        }
        if (found == 2 && s.ok) return INPUT_GENBANK;
    }
    // FASTA or plain sequence: only letters in the sequence lines, except for the end of a line
    const char *p = data.data(), *e = p + data.size();
    while (p < e) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
        const char *le = nl ? nl : e;
        if (*p != '>') {
            bool blank = false;
            for (const char *q = p; q < le; q++) {
                if (isspace((unsigned char)*q)) blank = true;
                else if (!isalpha((unsigned char)*q) && blank) { if (wrongChar) *wrongChar = *q; return INPUT_UNKNOWN; }
            }
        }
        p = nl ? nl + 1 : e;
    }
    return INPUT_FASTA;
}

bool readGenbank(const std::string &data, const GbOptions &go, GbFile &res, std::string &fatal) {
    const char *p = data.data(), *e = p + data.size();
    int annocount = 0;
    for (;;) {
        // reference GBSplitter::gotoEnd: the entry ends with the line whose first characters after blanks are "//"
        const char *q = p, *entryEnd = nullptr;
        while (q < e) {
            const char *nl = (const char *)memchr(q, '\n', (size_t)(e - q));
            const char *le = nl ? nl : e, *next = nl ? nl + 1 : e;
            const char *w = q;
            while (w < le && isspace((unsigned char)*w)) w++;
            if (w + 1 < le && w[0] == '/' && w[1] == '/') { entryEnd = next; break; }
            q = next;
        }
        if (!entryEnd) break; // no further entry (one that lacks its "//" line is not read)
        Positions pos;
        pos.buffer = p;
        pos.bufEnd = entryEnd;
        p = entryEnd;
        try {
            findPositions(pos, res);
            res.loci.push_back(getAnnoSequence(pos, go, res));
            annocount++;
        } catch (GbError &er) {
            res.err += "GBProcessor::getGeneList(): " + er.msg + "\nEncountered error after reading " + std::to_string(annocount) + " annotations.\n";
        }
    }
    if (annocount == 0) { fatal = "No genbank sequences found."; return false; }
    if (go.verbosity) res.out += "# Read in " + std::to_string(annocount) + " genbank sequences.\n";
    return true;
}

void printAnnotationGFF(std::string &out, const GbLocus &locus, const OutputOptions &o) {
    out += "# Sequence " + locus.name + " length=" + std::to_string(locus.length) + "\n";
    for (const Transcript &t : locus.genes) printTranscriptGFF(out, t, o, "database");
}

} // namespace augx
