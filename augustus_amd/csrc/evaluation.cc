// evaluation.cc -- see evaluation.h
#include "evaluation.h"
#include <algorithm>
#include <cstdlib>
#include <iomanip>
#include <sstream>

namespace augx {

using std::endl;
using std::setprecision;
using std::setw;

void Evaluation::add(const std::vector<Transcript> &predicted, const std::vector<Transcript> &annotated, int strand) {
    // the flanking regions on both sides of the annotated genes (any strand)
    leftFlankEnd = -1;
    rightFlankBegin = -1;
    for (const Transcript &a : annotated) {
        if ((leftFlankEnd == -1 && a.geneBegin() > 0) || (leftFlankEnd >= 0 && a.geneBegin() - 1 < leftFlankEnd)) leftFlankEnd = a.geneBegin() - 1;
        if (rightFlankBegin == -1 || a.geneEnd() + 1 > rightFlankBegin) rightFlankBegin = a.geneEnd() + 1;
    }
    if (rightFlankBegin == -1)
        for (const Transcript &p : predicted)
            if (p.geneEnd() + 1 > rightFlankBegin) rightFlankBegin = p.geneEnd() + 1;
    for (int plus = 1; plus >= 0; plus--) {
        if (strand != 0 && (strand > 0) != (plus == 1)) continue;
        std::vector<const Transcript *> pred, anno;
        for (const Transcript &t : predicted) if (t.plus == (plus == 1)) pred.push_back(&t);
        for (const Transcript &t : annotated) if (t.plus == (plus == 1)) anno.push_back(&t);
        addStrand(pred, anno);
    }
    numQuotients++;
}

static void sortUnique(std::vector<std::pair<long, long>> &v) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
}

void Evaluation::addStrand(const std::vector<const Transcript *> &pred, const std::vector<const Transcript *> &anno) {
    std::vector<Interval> pe, ae;
    for (const Transcript *g : pred) for (const BioState &s : g->exons) pe.push_back({s.begin, s.end});
    for (const Transcript *g : anno) for (const BioState &s : g->exons) ae.push_back({s.begin, s.end});
    numAnnoExons += (int)ae.size();
    numPredExons += (int)pe.size();
    sortUnique(pe);
    sortUnique(ae);
    numUniqueAnnoExons += (int)ae.size();
    numUniquePredExons += (int)pe.size();

    nucleotideLevel(pe, ae, false); // coding bases only
    exonLevel(pe, ae, false);
    geneLevel(pred, anno);
    utrLevel(pred, anno);

    // the derived values (0/0 stays what the division gives: the reference prints it)
    nukSens = (double)nukTP / (nukTP + nukFN);
    nukSpec = (double)nukTP / (nukTP + nukFP);
    exonFP = exonFP_wrong + exonFP_partial + exonFP_overlapping;
    exonFN = exonFN_wrong + exonFN_partial + exonFN_overlapping;
    exonSens = (double)exonTP / (exonTP + exonFN);
    exonSpec = (double)exonTP / (exonTP + exonFP);
    geneFP = numPredGenes - geneTP;
    geneSens = (double)geneTP / (geneTP + geneFN);
    geneSpec = (double)geneTP / (geneTP + geneFP);
    UTRexonSens = (double)UTRexonTP / (UTRexonTP + UTRexonFN);
    UTRexonSpec = (double)UTRexonTP / (UTRexonTP + UTRexonFP);
    nucUSens = (double)nucUTP / (nucUTP + nucUFN);
    nucUSpec = (double)nucUTP / (nucUTP + nucUFP);
    numDataSets++;
}

void Evaluation::nucleotideLevel(const std::vector<Interval> &pred, const std::vector<Interval> &anno, bool utr) {
    long n = 0;
    for (const Interval &a : anno) n = std::max(n, a.second);
    for (const Interval &p : pred) n = std::max(n, p.second);
    // per base: 1 annotated, 2 predicted, 4 predicted outside the flanking regions
    std::vector<char> nuc((size_t)n + 1, 0);
    for (const Interval &p : pred)
        for (long i = p.first >= 0 ? p.first : 0; i <= p.second; i++) {
            nuc[(size_t)i] |= 2;
            if (i > leftFlankEnd && i < rightFlankBegin) nuc[(size_t)i] |= 4;
        }
    for (const Interval &a : anno)
        for (long i = a.first >= 0 ? a.first : 0; i <= a.second; i++) nuc[(size_t)i] |= 1;
    int tp = 0, fp = 0, fpInside = 0, fn = 0;
    for (long i = 0; i <= n; i++) {
        const int f = nuc[(size_t)i];
        if (f == 1) fn++;
        if ((f & 1) == 0 && (f & 2)) fp++;
        if ((f & 1) == 0 && (f & 4)) fpInside++;
        if ((f & 1) && (f & 2)) tp++;
    }
    if (!utr) { nukFN += fn; nukFP += fp; nukFPinside += fpInside; nukTP += tp; }
    else { nucUFN += fn; nucUFP += fp; nucUFPinside += fpInside; nucUTP += tp; }
}

void Evaluation::exonLevel(const std::vector<Interval> &pred, const std::vector<Interval> &anno, bool utr) {
    // the best that can be said of an exon against the other set: 0 wrong, 1 overlaps, 2 one end exact, 3 both ends at most
    // UTRoffThresh off, 4 correct
    auto klasse = [&](const Interval &x, const std::vector<Interval> &others) {
        int k = 0;
        for (const Interval &o : others) {
            if (!(x.first > o.second || x.second < o.first) && k < 1) k = 1;
            if ((x.first == o.first || x.second == o.second) && k < 2) k = 2;
            if (std::labs(x.first - o.first) <= UTRoffThresh && std::labs(x.second - o.second) <= UTRoffThresh && k < 3) k = 3;
            if (x.first == o.first && x.second == o.second && k < 4) k = 4;
        }
        return k;
    };
    for (const Interval &x : pred)
        switch (klasse(x, anno)) {
        case 0: if (!utr) exonFP_wrong++; else UTRexonFP++; break;
        case 1: if (!utr) exonFP_overlapping++; else UTRexonFP++; break;
        case 2: if (!utr) exonFP_partial++; else UTRexonFP++; break;
        case 3: if (!utr) exonFP_partial++; else UTRexonTP++; break; // (UTR exons: less stringent)
        case 4: if (!utr) exonTP++; else UTRexonTP++; break;
        }
    for (const Interval &x : anno)
        switch (klasse(x, pred)) {
        case 0: if (!utr) exonFN_wrong++; else UTRexonFN++; break;
        case 1: if (!utr) exonFN_overlapping++; else UTRexonFN++; break;
        case 2: if (!utr) exonFN_partial++; else UTRexonFN++; break;
        case 3: if (!utr) exonFN_partial++; break;
        default: break; // (true positives were counted above: an exon may be annotated several times)
        }
}

static bool sameIntervals(const std::vector<BioState> &a, const std::vector<BioState> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].begin != b[i].begin || a[i].end != b[i].end) return false;
    return true;
}

void Evaluation::geneLevel(const std::vector<const Transcript *> &pred, const std::vector<const Transcript *> &anno) {
    for (const Transcript *a : anno) {
        numAnnoGenes++;
        bool correct = false;
        for (const Transcript *p : pred)
            if (sameIntervals(a->exons, p->exons) && p->complete) { correct = true; break; }
        if (correct) geneTP++; else geneFN++;
    }
    // the number of distinct predicted transcripts (exons, introns and UTR exons: reference Transcript::operator==)
    for (size_t i = 0; i < pred.size(); i++) {
        bool seen = false;
        for (size_t k = 0; k < i && !seen; k++)
            seen = sameIntervals(pred[k]->exons, pred[i]->exons) && sameIntervals(pred[k]->introns, pred[i]->introns) &&
                   sameIntervals(pred[k]->utr5exons, pred[i]->utr5exons) && sameIntervals(pred[k]->utr3exons, pred[i]->utr3exons);
        if (!seen) numPredGenes++;
    }
}

void Evaluation::utrLevel(const std::vector<const Transcript *> &pred, const std::vector<const Transcript *> &anno) {
    // predicted transcription starts against the annotated genes with the same translation start, then the same for the ends
    for (const Transcript *p : pred) {
        const long predTSS = p->plus ? p->transstart : p->transend, predTIS = p->plus ? p->codingstart : p->codingend;
        if (predTSS >= 0 && p->complete5utr) {
            numTotalPredTSS++;
            for (const Transcript *a : anno) {
                const long annoTSS = a->plus ? a->transstart : a->transend, annoTIS = a->plus ? a->codingstart : a->codingend;
                if (annoTIS == predTIS && annoTSS >= 0) {
                    const long diff = std::labs(predTSS - annoTSS);
                    numTSS++;
                    if (diff <= MAXUTRDIST) tssDist[(size_t)diff]++;
                }
            }
        }
    }
    for (const Transcript *p : pred) {
        const long predTTS = p->plus ? p->transend : p->transstart, predSTP = p->plus ? p->codingend : p->codingstart;
        if (predTTS >= 0 && p->complete3utr) {
            numTotalPredTTS++;
            for (const Transcript *a : anno) {
                const long annoTTS = a->plus ? a->transend : a->transstart, annoSTP = a->plus ? a->codingend : a->codingstart;
                if (annoSTP == predSTP && annoTTS >= 0) {
                    const long diff = std::labs(predTTS - annoTTS);
                    numTTS++;
                    if (diff <= MAXUTRDIST) ttsDist[(size_t)diff]++;
                }
            }
        }
    }
    std::vector<Interval> pe, ae;
    for (const Transcript *g : pred) {
        for (const BioState &s : g->utr5exons) pe.push_back({s.begin, s.end});
        for (const BioState &s : g->utr3exons) pe.push_back({s.begin, s.end});
    }
    for (const Transcript *g : anno) {
        for (const BioState &s : g->utr5exons) ae.push_back({s.begin, s.end});
        for (const BioState &s : g->utr3exons) ae.push_back({s.begin, s.end});
    }
    numAnnoUTRExons += (int)ae.size();
    numPredUTRExons += (int)pe.size();
    sortUnique(pe);
    sortUnique(ae);
    numUniqueAnnoUTRExons += (int)ae.size();
    numUniquePredUTRExons += (int)pe.size();
    exonLevel(pe, ae, true);
    nucleotideLevel(pe, ae, true);
}

void Evaluation::finishAndPrint(std::string &text) {
    std::ostringstream out;
    // ---- finishEvaluation: mean and median distance of the predicted transcription starts and ends
    auto finish = [&](const char *what, int num, const std::vector<int> &dist, double &mean, int &median) {
        if (num > 0) {
            mean = 0.0;
            int numInRange = 0, cumNum = 0;
            median = -1;
            out << what << " distances " << endl;
            for (int i = 0; i <= MAXUTRDIST; i++)
                if (dist[(size_t)i] > 0) {
                    cumNum += dist[(size_t)i];
                    if (2 * cumNum >= num && median < 0) median = i;
                    mean += i * dist[(size_t)i];
                    numInRange += dist[(size_t)i];
                    out << i << "\ttimes:" << dist[(size_t)i] << endl;
                }
            if (num - numInRange > 0) out << "Warning: " << num - numInRange << " " << what << " are off by more than " << (int)MAXUTRDIST << endl;
            mean += MAXUTRDIST * (num - numInRange); // (every distance beyond MAXUTRDIST counts as MAXUTRDIST)
            mean /= num;
        } else {
            median = -1;
            mean = -1;
        }
    };
    finish("TSS", numTSS, tssDist, meanTssDist, medianTssDist);
    finish("TTS", numTTS, ttsDist, meanTtsDist, medianTtsDist);
    // ---- printQuotients: the quotient of path probabilities is 0 for every locus of a prediction run
    out << "a-posteriori probability of viterbi path" << endl;
    out << "----------------------------------------" << endl;
    out << "a-posteriori probability of correct path" << endl << endl;
    out << numQuotients << " times were the paths equally likely (identical)." << endl;
    out << "sorted quotients of the rest:" << endl;
    out << endl << 0 << " quotients were between 1 and 10" << endl;
    out << endl;
    // ---- print
    out << "\n*******      Evaluation of gene prediction     *******" << endl << endl;
    out << "---------------------------------------------\\" << endl;
    out << setw(16) << " " << " | " << setw(11) << "sensitivity" << " | " << setw(11) << "specificity" << " |" << endl;
    out << "---------------------------------------------|" << endl;
    out << setw(16) << "nucleotide level" << " | " << setw(11) << setprecision(3) << nukSens << " | " << setw(11) << setprecision(3) << nukSpec << " |" << endl;
    out << "---------------------------------------------/" << endl << endl;
    // exon level
    out << "-----------------------------------------------------------------------------" << "-----------------------------\\" << endl;
    out << setw(10) << " " << " | " << setw(6) << "#pred" << " | " << setw(6) << "#anno" << " | " << setw(4) << " " << " | " << setw(18) << "FP = false pos."
        << " | " << setw(18) << "FN = false neg." << " | " << setw(11) << " " << " | " << setw(11) << " " << " |" << endl;
    out << setw(10) << " " << " | " << setw(6) << "total/" << " | " << setw(6) << "total/" << " | " << setw(4) << "TP" << " |" << setw(19) << "--------------------"
        << "|" << setw(19) << "--------------------" << "| " << setw(11) << "sensitivity" << " | " << setw(11) << "specificity" << " |" << endl;
    out << setw(10) << " " << " | " << setw(6) << "unique" << " | " << setw(6) << "unique" << " | " << setw(4) << " " << " | " << setw(4) << "part" << " | " << setw(4)
        << "ovlp" << " | " << setw(4) << "wrng" << " | " << setw(4) << "part" << " | " << setw(4) << "ovlp" << " | " << setw(4) << "wrng" << " | " << setw(11) << " "
        << " | " << setw(11) << " " << " |" << endl;
    out << "-----------------------------------------------------------------------------" << "-----------------------------|" << endl;
    out << setw(10) << " " << " | " << setw(6) << " " << " | " << setw(6) << " " << " | " << setw(4) << " " << " | " << setw(18) << exonFP << " | " << setw(18) << exonFN
        << " | " << setw(11) << " " << " | " << setw(11) << " " << " |" << endl;
    out << setw(10) << "exon level" << " | " << setw(6) << numPredExons << " | " << setw(6) << numAnnoExons << " | " << setw(4) << exonTP << " | " << setw(18)
        << "------------------" << " | " << setw(18) << "------------------" << " | " << setw(11) << setprecision(3) << exonSens << " | " << setw(11) << setprecision(3)
        << exonSpec << " |" << endl;
    out << setw(10) << " " << " | " << setw(6) << numUniquePredExons << " | " << setw(6) << numUniqueAnnoExons << " | " << setw(4) << " " << " | " << setw(4)
        << exonFP_partial << " | " << setw(4) << exonFP_overlapping << " | " << setw(4) << exonFP_wrong << " | " << setw(4) << exonFN_partial << " | " << setw(4)
        << exonFN_overlapping << " | " << setw(4) << exonFN_wrong << " | " << setw(11) << " " << " | " << setw(11) << " " << " |" << endl;
    out << "-----------------------------------------------------------------------------" << "-----------------------------/" << endl << endl;
    // transcript level
    out << "-----------------------------------------------------" << "-----------------------\\" << endl;
    out << setw(10) << "transcript" << " | " << setw(5) << "#pred" << " | " << setw(5) << "#anno" << " | " << setw(4) << "TP" << " | " << setw(4) << "FP" << " | " << setw(4)
        << "FN" << " | " << setw(11) << "sensitivity" << " | " << setw(9) << "specificity" << " |" << endl;
    out << "------------------------------------------------------" << "----------------------|" << endl;
    out << setw(10) << "gene level" << " | " << setw(5) << numPredGenes << " | " << setw(5) << numAnnoGenes << " | " << setw(4) << geneTP << " | " << setw(4) << geneFP << " | "
        << setw(4) << geneFN << " | " << setw(11) << setprecision(3) << geneSens << " | " << setw(11) << setprecision(3) << geneSpec << " |" << endl;
    out << "-------------------------------------------------------" << "---------------------/" << endl;
    if (numTotalPredTSS > 0 || numTotalPredTTS > 0) {
        out << endl;
        out << "------------------------------------------------------------------------\\" << endl;
        out << setw(15) << "UTR" << " | " << setw(10) << "total pred" << " | " << setw(14) << "CDS bnd. corr." << " | " << setw(10) << "meanDiff" << " | " << setw(10)
            << "medianDiff" << " |" << endl;
        out << "------------------------------------------------------------------------|" << endl;
        out << setw(15) << "TSS" << " | " << setw(10) << numTotalPredTSS << " | " << setw(14) << numTSS << " | " << setw(10) << setprecision(3) << meanTssDist << " | "
            << setw(10) << medianTssDist << " |" << endl;
        out << setw(15) << "TTS" << " | " << setw(10) << numTotalPredTTS << " | " << setw(14) << numTTS << " | " << setw(10) << setprecision(3) << meanTtsDist << " | "
            << setw(10) << medianTtsDist << " |" << endl;
        out << "------------------------------------------------------------------------|" << endl;
        out << setw(15) << "UTR" << " | " << setw(10) << "uniq. pred" << " | " << setw(14) << "unique anno" << " | " << setw(10) << "   sens." << " | " << setw(10)
            << "     spec." << " |" << endl;
        out << "------------------------------------------------------------------------|" << endl;
        out << setw(15) << " " << " | " << setw(45) << "true positive = 1 bound. exact, 1 bound. <= " << UTRoffThresh << "bp off" " |" << endl;
        out << setw(15) << "UTR exon level" << " | " << setw(10) << numUniquePredUTRExons << " | " << setw(14) << numUniqueAnnoUTRExons << " | " << setw(10)
            << setprecision(3) << UTRexonSens << " | " << setw(10) << UTRexonSpec << " |" << endl;
        out << "------------------------------------------------------------------------|" << endl;
        out << setw(15) << "UTR base level" << " | " << setw(10) << (nucUTP + nucUFP) << " | " << setw(14) << (nucUTP + nucUFN) << " | " << setw(10) << setprecision(3)
            << nucUSens << " | " << setw(10) << nucUSpec << " |" << endl;
        out << "------------------------------------------------------------------------/" << endl;
        out << "nucUTP= " << nucUTP << " nucUFP=" << nucUFP << " nucUFPinside= " << nucUFPinside << " nucUFN=" << nucUFN << endl;
    }
    text += out.str();
}

} // namespace augx
