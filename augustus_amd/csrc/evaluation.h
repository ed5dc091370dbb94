// evaluation.h -- accuracy of predicted against annotated transcripts, and the report the reference prints after a run on
// GenBank input.  Restates what the ab-initio run uses of the reference's Evaluation (include/evaluation.hh, src/evaluation.cc):
// addToEvaluation (:18-163), the nucleotide (:234-306), exon (:376-457), transcript (:496-537) and UTR level (:539-666),
// finishEvaluation (:668-720), printQuotients (:822-841) and print (:722-820).  The accuracy of extrinsic evidence is not built.
#pragma once
#include <string>
#include <vector>
#include "genes.h"

namespace augx {

class Evaluation {
public:
    enum { MAXUTRDIST = 5000 };
    Evaluation() : tssDist(MAXUTRDIST + 1, 0), ttsDist(MAXUTRDIST + 1, 0) {}
    // one locus; strand: 0 both, +1 forward only, -1 reverse only (--strand)
    void add(const std::vector<Transcript> &predicted, const std::vector<Transcript> &annotated, int strand);
    // the lines about TSS / TTS distances, the block of path quotients and the tables, as the reference prints them in this order
    void finishAndPrint(std::string &out);

    // nucleotide level
    int nukTP = 0, nukFP = 0, nukFN = 0, nukFPinside = 0;
    int nucUTP = 0, nucUFP = 0, nucUFN = 0, nucUFPinside = 0;
    double nukSens = 0, nukSpec = 0, nucUSens = 0, nucUSpec = 0, exonSens = 0, exonSpec = 0, UTRexonSens = 0, UTRexonSpec = 0, geneSens = 0, geneSpec = 0;
    // exon level
    int numPredExons = 0, numAnnoExons = 0, numUniquePredExons = 0, numUniqueAnnoExons = 0;
    int exonTP = 0, exonFP = 0, exonFP_partial = 0, exonFP_overlapping = 0, exonFP_wrong = 0, exonFN = 0, exonFN_partial = 0, exonFN_overlapping = 0,
        exonFN_wrong = 0;
    // transcript level
    int geneTP = 0, geneFP = 0, geneFN = 0, numPredGenes = 0, numAnnoGenes = 0;
    // UTR level
    int numTSS = 0, numTotalPredTSS = 0, medianTssDist = -1, numTTS = 0, numTotalPredTTS = 0, medianTtsDist = -1;
    double meanTssDist = -1, meanTtsDist = -1;
    int numPredUTRExons = 0, numAnnoUTRExons = 0, numUniquePredUTRExons = 0, numUniqueAnnoUTRExons = 0;
    int UTRexonTP = 0, UTRexonFP = 0, UTRexonFN = 0;
    int UTRoffThresh = 20; // a UTR exon counts as correct when both ends are at most this many bases off
    int numDataSets = 0;   // strands evaluated
    int numQuotients = 0;  // loci added (the reference keeps one quotient of path probabilities per locus, 0 in this mode)

private:
    typedef std::pair<long, long> Interval;
    void addStrand(const std::vector<const Transcript *> &pred, const std::vector<const Transcript *> &anno);
    void nucleotideLevel(const std::vector<Interval> &pred, const std::vector<Interval> &anno, bool utr);
    void exonLevel(const std::vector<Interval> &pred, const std::vector<Interval> &anno, bool utr);
    void geneLevel(const std::vector<const Transcript *> &pred, const std::vector<const Transcript *> &anno);
    void utrLevel(const std::vector<const Transcript *> &pred, const std::vector<const Transcript *> &anno);
    long leftFlankEnd = -1, rightFlankBegin = -1;
    std::vector<int> tssDist, ttsDist;
};

} // namespace augx
