// bcd_cli.cpp -- command-line front-end with the reference's flags, defaults and file conventions
// (src/cli/main.cpp:122-504 of the reference): -o -i -h -c -d -b -w -r -p --p-factor -m -s --ncores --use-cuda -e.
// Real defaults are -r 1 and -p 1 (main.cpp:52-53) although the reference's README says 0.  Missing -h / -c are
// inferred as <input>_hist.exr / <input>_cov.exr (:344-370).  Extra flags of this build: --seed <n> (visiting
// order), --device <n>.  --ncores only selects the visiting order (n > 1 with -r 0: the reference's strip list; the loop runs on the HIP device); --use-cuda 0 (a request for the CPU path this
// build does not have) is declined with a note and served by the device; under BCD_STRICT_CPU_REQUEST=1 it is refused with an error before any file is read.
// --layer <color.exr> <cov.exr> <out.exr> (repeatable) denoises a further colour layer with the filter of the -i image (one selection of similar patches for all).
// --neighbour-layer <color.exr> <cov.exr> hands the most recent --neighbour the matching layer (the k-th pairs with the k-th --layer).
// --neighbour-motion <mv.exr> hands the most recent --neighbour its motion field ((dx, dy) in the first two channels).
// --neighbour-nsamples <file|n> hands the most recent --neighbour its sample counts under --moment-selection, where no <frame>_hist.exr is loaded.
// --neighbour-features <f.exr> / --neighbour-feature-variances <v.exr> hand the most recent --neighbour its feature buffers: with --features the gate covers
// the search in the neighbours too (every neighbour then needs them).
// -a <file.bcd.json> (advertised but never parsed by the reference, main.cpp:107) loads a preset; later flags override it.
// --sequence-in <pattern with %d> --sequence-out <pattern with %d> --first a --last b --temporal-radius R denoises the frames a .. b of an animation, each with
// its neighbours within R frames, through bcd::SequenceDenoiser (every frame uploaded once, every pair of frames searched once); it replaces -i / -o.
// Beside it --sequence-layer <colours> <covariances> <output> (patterns), --sequence-moments <floor> --sequence-nsamples <pattern> and --sequence-features
// <pattern> with --sequence-feature-variances / -floors / -threshold give every frame its colour layers, the moment selection and the feature gate.
// --sequence-motion-prev <pattern> and --sequence-motion-next <pattern> give every frame its motion field towards the frame before and after it
// (SequenceDenoiser::setFrameMotion); the file of the first frame (prev) and of the last frame (next) may be missing.
#include "Chronometer.h"
#include "DeepImage.h"
#include "Denoiser.h"
#include "ImageIO.h"
#include "MultiscaleDenoiser.h"
#include "ParametersIO.h"
#include "SequenceDenoiser.h"
#include "SpikeRemovalFilter.h"
#include "Utils.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>
#include <memory>
#include <string>

using namespace std;
using namespace bcd;

namespace
{

	struct ProgramArguments
	{
		string m_denoisedOutputFilePath;
		Deepimf m_colorImage, m_nbOfSamplesImage, m_histogramImage, m_covarianceImage;
		float m_histogramPatchDistanceThreshold = 1.f;
		int m_patchRadius = 1;
		int m_searchWindowRadius = 6;
		float m_minEigenValue = 1.e-8f;
		bool m_useRandomPixelOrder = true;
		bool m_prefilterSpikes = true;
		float m_prefilterThresholdStDevFactor = 2.f;
		float m_markedPixelsSkippingProbability = 1.f;
		int m_nbOfScales = 3;
		int m_nbOfCores = 0;
		bool m_useCuda = true;
		unsigned m_orderSeed = 1234u;
		std::vector<int> m_devices = std::vector<int>(1, 0);
		struct Layer { string m_colorPath, m_covariancePath, m_outputPath; Deepimf m_colorImage, m_covarianceImage; };
		struct NeighbourLayer { string m_colorPath, m_covariancePath; Deepimf m_colorImage, m_covarianceImage; };
		struct Neighbour { string m_nbOfSamplesArgument; /* --neighbour-nsamples */ string m_colorPath; Deepimf m_colorImage, m_nbOfSamplesImage, m_histogramImage, m_covarianceImage; std::vector<NeighbourLayer> m_layers; /* --neighbour-layer */ string m_motionPath; Deepimf m_motionImage; /* --neighbour-motion */ string m_featurePath, m_featureVariancePath; Deepimf m_featureImage, m_featureVarianceImage; /* --neighbour-features, --neighbour-feature-variances */ };
		std::vector<Neighbour> m_neighbours; // --neighbour, in command-line order
		std::vector<Layer> m_layers; // --layer, in command-line order
		bool m_prefilterFrames = false; // --prefilter-frames: -p 1 beside --neighbour* or --sequence-in, every frame prefiltered on its own (setSpikePrefilterFrames)
		bool m_prefilterLayers = false; // --prefilter-layers: -p 1 beside --layer, every layer gathered through the decision taken on the -i colours
		bool m_momentSelection = false; // --moment-selection: similar patches from the -i colours and the -c covariances, no histogram file
		float m_momentVarianceFloor = 1.e-8f;
		string m_featurePath, m_featureVariancePath; // --features / --feature-variances: auxiliary buffers that gate the similar-patch selection
		Deepimf m_featureImage, m_featureVarianceImage;
		std::vector<float> m_featureFloors;          // --feature-floors: one per channel
		float m_featureThreshold = 1.f;              // --feature-threshold
	};

	const char* g_pProgramPath = "bcd_cli";

	void printUsage()
	{
		ProgramArguments d;
		cout << "Bayesian Collaborative Denoising (MI355X / HIP build)" << endl << endl;
		cout << "Usage: " << g_pProgramPath << " <arguments list>" << endl;
		cout << "Only EXR images are supported." << endl << endl;
		cout << "Required arguments list:" << endl;
		cout << "    -o <output>          The file path to the output image" << endl;
		cout << "    -i <input>           The file path to the input image" << endl;
		cout << "    -h <hist>            The file path to the input histograms buffer (default: <input>_hist.exr)" << endl;
		cout << "    -c <cov>             The file path to the input covariance matrices buffer (default: <input>_cov.exr)" << endl;
		cout << "Optional arguments list:" << endl;
		cout << "    -a <file>            The file path to the .bcd.json file containing arguments for the program" << endl;
		cout << "    --neighbour <frame>  A neighbouring frame of the sequence that lends its statistics (repeatable, at most 4; expects <frame>_hist.exr / <frame>_cov.exr beside it)" << endl;
		cout << "    --neighbour-nsamples <file|n>" << endl;
		cout << "                         with --moment-selection (no <frame>_hist.exr is loaded then): the sample counts of the most recent --neighbour, a" << endl;
		cout << "                         one-channel EXR image or one number for every pixel; without it a numeric --nsamples serves every neighbour" << endl;
		cout << "    --neighbour-motion <mv.exr>" << endl;
		cout << "                         the motion field of the most recent --neighbour: pixel (x, y) of the frame shows what pixel (x + dx, y + dy) of that" << endl;
		cout << "                         neighbour shows, (dx, dy) in the first two channels, rounded to whole pixels; NaN marks a disoccluded pixel" << endl;
		cout << "    --neighbour-features <file>" << endl;
		cout << "                         the feature buffers of the most recent --neighbour, channels as --features: with --features every neighbour needs" << endl;
		cout << "                         them, and a patch of a neighbour stays similar only if its features agree with the frame's" << endl;
		cout << "    --neighbour-feature-variances <file>" << endl;
		cout << "                         the variances of that neighbour's features (given exactly when --feature-variances is)" << endl;
		cout << "    --neighbour-layer <color> <cov>" << endl;
		cout << "                         a colour layer of the most recent --neighbour: the k-th one pairs with the k-th --layer; every neighbour" << endl;
		cout << "                         needs exactly one per --layer (one selection over all frames then serves every layer; needs -p 0 or --prefilter-frames)" << endl;
		cout << "    --sequence-in <pattern> --sequence-out <pattern> --first <a> --last <b> [--temporal-radius <R>]" << endl;
		cout << "                         in place of -i / -o: the frames a .. b of an animation, the patterns holding one %d (or %04d ...) for the frame number;" << endl;
		cout << "                         every frame is denoised with its neighbours within R frames (1 or 2, default 1) and written to its output name." << endl;
		cout << "                         Expects <frame>_hist.exr / <frame>_cov.exr beside every input, as --neighbour does; needs -p 0 or --prefilter-frames, -w 1, -b 6 and a single" << endl;
		cout << "                         device; not with -i, -o, -h, -c, --neighbour, --layer, --features or --moment-selection" << endl;
		cout << "    --sequence-layer <colours pattern> <covariances pattern> <output pattern>" << endl;
		cout << "                         beside --sequence-in: a further colour layer of every frame (repeatable, at most 15), denoised with the frame's selection" << endl;
		cout << "    --sequence-motion-prev <pattern> --sequence-motion-next <pattern>" << endl;
		cout << "                         beside --sequence-in: the motion field of every frame towards the frame before it / after it ((dx, dy) in the first two" << endl;
		cout << "                         channels, as --neighbour-motion); a neighbour frame is warped by the field, fields two frames away are composed from" << endl;
		cout << "                         the steps.  The file of frame --first (prev) and of frame --last (next) may be missing: zero motion" << endl;
		cout << "    --sequence-moments <var floor> --sequence-nsamples <pattern>" << endl;
		cout << "                         beside --sequence-in: every selection from means and covariances; no <frame>_hist.exr is read, the sample counts of" << endl;
		cout << "                         every frame come from a one-channel EXR image" << endl;
		cout << "    --sequence-features <pattern> --sequence-feature-floors <a,b,...> [--sequence-feature-variances <pattern>] [--sequence-feature-threshold <float>]" << endl;
		cout << "                         beside --sequence-in: the feature buffers of every frame gate the selection inside the frame and across frames," << endl;
		cout << "                         with the meanings of --features, --feature-floors, --feature-variances and --feature-threshold" << endl;
		cout << "    -d <float>           Histogram patch distance threshold (default: " << d.m_histogramPatchDistanceThreshold << ")" << endl;
		cout << "    -b <int>             Radius of search windows (default: " << d.m_searchWindowRadius << ")" << endl;
		cout << "    -w <int>             Radius of patches (default: " << d.m_patchRadius << ")" << endl;
		cout << "    -r <0/1>             1 for random pixel order (in case of grid artifacts) (default: " << (d.m_useRandomPixelOrder ? 1 : 0) << ")" << endl;
		cout << "    -p <0/1>             1 for a spike removal prefiltering (default: " << (d.m_prefilterSpikes ? 1 : 0) << ")" << endl;
		cout << "    --p-factor <float>   Standard deviation factor of the spike threshold (default: " << d.m_prefilterThresholdStDevFactor << ")" << endl;
		cout << "    -m <float in [0,1]>  Probability of skipping marked centers of denoised patches (default: " << d.m_markedPixelsSkippingProbability << ")" << endl;
		cout << "    -s <int>             Number of Scales for Multi-Scaling (default: " << d.m_nbOfScales << ")" << endl;
		cout << "    --ncores <n>         the loop runs on the HIP device; n > 1 with -r 0 selects the reference's strip visiting order" << endl;
		cout << "    --use-cuda <0/1>     1 (default): run on the HIP device; 0 asks for the CPU path, which this build does not have: declined with a note, the device runs (BCD_STRICT_CPU_REQUEST=1: refused)" << endl;
		cout << "    -e <float>           Minimum eigen value for matrix inversion (default: " << d.m_minEigenValue << ")" << endl;
		cout << "    --seed <int>         Seed of the random pixel order (default: " << d.m_orderSeed << ")" << endl;
		cout << "    --device <int>       HIP device index (default: 0)" << endl;
		cout << "    --devices <list>     several HIP devices, e.g. 0-7 or 0,2,4: the frame is split into row bands (RCCL halo exchange)" << endl;
		cout << "    --layer <color> <cov> <output>" << endl;
		cout << "                         a further colour layer (light group, diffuse / specular pass, ...) of the same render: its mean colours and" << endl;
		cout << "                         sample covariances, denoised with the similar patches of the -i image and written to <output>; repeatable" << endl;
		cout << "                         (at most 15), shares -h; needs a single device, and -p 0 or --prefilter-layers" << endl;
		cout << "    --prefilter-layers   with -p 1 (given or by default) and --layer: the spike prefilter decides on the -i colours which neighbour" << endl;
		cout << "                         replaces a pixel, and every layer's colours and covariances are gathered through that decision on the device;" << endl;
		cout << "                         no effect with -p 0" << endl;
		cout << "    --prefilter-frames   with -p 1 (given or by default) beside --neighbour* or --sequence-in: every frame -- the -i frame and each neighbour," << endl;
		cout << "                         every frame of a sequence -- passes through the spike prefilter on its own, all its layers following the decision" << endl;
		cout << "                         taken on its own colours; feature buffers and motion fields are not moved; no effect with -p 0" << endl;
		cout << "    --moment-selection [floor]" << endl;
		cout << "                         select similar patches from the -i colours and the -c covariances instead of histograms: no histogram file is" << endl;
		cout << "                         looked for, -d then thresholds the variance-normalised squared difference of the pixel means (1 on average between" << endl;
		cout << "                         pixels of equal signal); floor (default " << d.m_momentVarianceFloor << ") is added to every summed variance.  Needs the" << endl;
		cout << "                         sample counts from --nsamples (or from a -h file, whose histograms are then ignored) and a single device" << endl;
		cout << "    --nsamples <file|n>  with --moment-selection: the sample counts, a one-channel EXR image or one number for every pixel" << endl;
		cout << "    --features <file>    auxiliary feature buffers (albedo, normal, depth, object id, ...: a multi-channel float EXR of 1 to 8 channels): two" << endl;
		cout << "                         patches stay similar only if their features agree as well, so nothing is averaged across an edge that only the" << endl;
		cout << "                         features show.  Needs --feature-floors and a single device" << endl;
		cout << "    --feature-variances <file>" << endl;
		cout << "                         the variance of every pixel's feature mean, same channels as --features (default: none)" << endl;
		cout << "    --feature-floors <a,b,...>" << endl;
		cout << "                         one non-negative number per feature channel, added to the summed variances; without variances the squared" << endl;
		cout << "                         tolerance of the channel (0.01: features within 0.1 agree), 0 switches the channel off" << endl;
		cout << "    --feature-threshold <float>" << endl;
		cout << "                         threshold of the mean squared normalised feature difference over a patch (default: " << d.m_featureThreshold << ")" << endl;
	}

	bool badValue(const char* flag, const char* what)
	{
		cout << "ERROR in program arguments: " << what << " after " << flag << endl;
		return false;
	}

	bool parseProgramArguments(int argc, const char** argv, ProgramArguments& a)
	{
		bool missingColor = true, missingHist = true, missingCov = true, missingOutput = true;
		string inputColorFilePath, nbOfSamplesArgument;
		for(int i = 1; i < argc; ++i)
		{
			const string flag = argv[i];
			if(flag == "--help") { printUsage(); return false; }
			if(flag == "--prefilter-layers") { a.m_prefilterLayers = true; continue; }
			if(flag == "--prefilter-frames") { a.m_prefilterFrames = true; continue; }
			if(flag == "--moment-selection")
			{
				a.m_momentSelection = true;
				char* pEnd = nullptr;
				const float floor = i + 1 < argc ? strtof(argv[i + 1], &pEnd) : 0.f;
				if(i + 1 < argc && pEnd != argv[i + 1] && *pEnd == '\0')
				{	// the optional value: a number
					if(!(floor >= 0.f) || std::isinf(floor)) return badValue("--moment-selection", "expecting a finite non-negative floating number");
					a.m_momentVarianceFloor = floor;
					++i;
				}
				continue;
			}
			if(flag == "--neighbour")
			{	// a neighbouring frame of the sequence: <frame>.exr with <frame>_hist.exr and <frame>_cov.exr beside it, as -i infers them
				if(i + 1 >= argc) { cout << "ERROR in program arguments: expecting <frame.exr> after --neighbour" << endl; return false; }
				a.m_neighbours.emplace_back();
				ProgramArguments::Neighbour& rNb = a.m_neighbours.back();
				rNb.m_colorPath = argv[++i];
				if(rNb.m_colorPath.length() <= 4) { cout << "ERROR in program arguments: '" << rNb.m_colorPath << "' is no .exr file name" << endl; return false; }
				const string stem = rNb.m_colorPath.substr(0, rNb.m_colorPath.length() - 4);
				// (its histograms and sample counts are loaded once the whole command line is read: under --moment-selection there is no <frame>_hist.exr)
				if(!ImageIO::loadEXR(rNb.m_colorImage, rNb.m_colorPath.c_str())) { cout << "ERROR in program arguments: couldn't load neighbour color image file '" << rNb.m_colorPath << "'" << endl; return false; }
				if(!ImageIO::loadMultiChannelsEXR(rNb.m_covarianceImage, (stem + "_cov.exr").c_str())) { cout << "ERROR in program arguments: couldn't load neighbour covariance matrix image file '" << stem << "_cov.exr'" << endl; return false; }
				continue;
			}
			if(flag == "--neighbour-nsamples")
			{	// with --moment-selection: the sample counts of the most recent --neighbour, a one-channel EXR image or one number for every pixel
				if(i + 1 >= argc) { cout << "ERROR in program arguments: expecting <file|n> after --neighbour-nsamples" << endl; return false; }
				if(a.m_neighbours.empty()) { cout << "ERROR in program arguments: --neighbour-nsamples follows the --neighbour it belongs to" << endl; return false; }
				a.m_neighbours.back().m_nbOfSamplesArgument = argv[++i];
				continue;
			}
			if(flag == "--neighbour-motion")
			{	// the motion field of the most recent --neighbour: (dx, dy) in the first two channels
				if(i + 1 >= argc) { cout << "ERROR in program arguments: expecting <mv.exr> after --neighbour-motion" << endl; return false; }
				if(a.m_neighbours.empty()) { cout << "ERROR in program arguments: --neighbour-motion follows the --neighbour it belongs to" << endl; return false; }
				ProgramArguments::Neighbour& rNb = a.m_neighbours.back();
				rNb.m_motionPath = argv[++i];
				Deepimf loaded;
				if(!ImageIO::loadMultiChannelsEXR(loaded, rNb.m_motionPath.c_str())) { cout << "ERROR in program arguments: couldn't load neighbour motion image file '" << rNb.m_motionPath << "'" << endl; return false; }
				if(loaded.getDepth() < 2) { cout << "ERROR in program arguments: neighbour motion image '" << rNb.m_motionPath << "' needs two channels (dx, dy)" << endl; return false; }
				rNb.m_motionImage.resize(loaded.getWidth(), loaded.getHeight(), 2);
				for(int px = 0, n = loaded.getWidth() * loaded.getHeight(), d = loaded.getDepth(); px < n; ++px)
				{
					rNb.m_motionImage.get(2 * px) = loaded.get(d * px);
					rNb.m_motionImage.get(2 * px + 1) = loaded.get(d * px + 1);
				}
				continue;
			}
			if(flag == "--neighbour-features" || flag == "--neighbour-feature-variances")
			{	// the feature buffers of the most recent --neighbour
				const bool variances = flag == "--neighbour-feature-variances";
				if(i + 1 >= argc) { cout << "ERROR in program arguments: expecting <file.exr> after " << flag << endl; return false; }
				if(a.m_neighbours.empty()) { cout << "ERROR in program arguments: " << flag << " follows the --neighbour it belongs to" << endl; return false; }
				ProgramArguments::Neighbour& rNb = a.m_neighbours.back();
				string& rPath = variances ? rNb.m_featureVariancePath : rNb.m_featurePath;
				rPath = argv[++i];
				if(!ImageIO::loadMultiChannelsEXR(variances ? rNb.m_featureVarianceImage : rNb.m_featureImage, rPath.c_str()))
				{
					cout << "ERROR in program arguments: couldn't load neighbour feature " << (variances ? "variance " : "") << "image file '" << rPath << "'" << endl;
					return false;
				}
				continue;
			}
			if(flag == "--neighbour-layer")
			{	// a colour layer of the most recent --neighbour: the k-th one pairs with the k-th --layer
				if(i + 2 >= argc) { cout << "ERROR in program arguments: expecting <color.exr> <cov.exr> after --neighbour-layer" << endl; return false; }
				if(a.m_neighbours.empty()) { cout << "ERROR in program arguments: --neighbour-layer follows the --neighbour it belongs to" << endl; return false; }
				a.m_neighbours.back().m_layers.emplace_back();
				ProgramArguments::NeighbourLayer& rLayer = a.m_neighbours.back().m_layers.back();
				rLayer.m_colorPath = argv[i + 1]; rLayer.m_covariancePath = argv[i + 2];
				i += 2;
				if(!ImageIO::loadEXR(rLayer.m_colorImage, rLayer.m_colorPath.c_str())) { cout << "ERROR in program arguments: couldn't load neighbour layer color image file '" << rLayer.m_colorPath << "'" << endl; return false; }
				if(!ImageIO::loadMultiChannelsEXR(rLayer.m_covarianceImage, rLayer.m_covariancePath.c_str())) { cout << "ERROR in program arguments: couldn't load neighbour layer covariance matrix image file '" << rLayer.m_covariancePath << "'" << endl; return false; }
				continue;
			}
			if(flag == "--layer")
			{
				if(i + 3 >= argc) { cout << "ERROR in program arguments: expecting <color.exr> <cov.exr> <output.exr> after --layer" << endl; return false; }
				a.m_layers.emplace_back();
				ProgramArguments::Layer& rLayer = a.m_layers.back();
				rLayer.m_colorPath = argv[i + 1]; rLayer.m_covariancePath = argv[i + 2]; rLayer.m_outputPath = argv[i + 3];
				i += 3;
				if(!ImageIO::loadEXR(rLayer.m_colorImage, rLayer.m_colorPath.c_str())) { cout << "ERROR in program arguments: couldn't load layer color image file '" << rLayer.m_colorPath << "'" << endl; return false; }
				if(!ImageIO::loadMultiChannelsEXR(rLayer.m_covarianceImage, rLayer.m_covariancePath.c_str())) { cout << "ERROR in program arguments: couldn't load layer covariance matrix image file '" << rLayer.m_covariancePath << "'" << endl; return false; }
				continue;
			}
			if(i + 1 >= argc) { cout << "ERROR in program arguments: expecting a value after " << flag << endl; return false; }
			const char* value = argv[++i];
			if(flag == "-o") { a.m_denoisedOutputFilePath = value; missingOutput = false; }
			else if(flag == "-i")
			{
				inputColorFilePath = value;
				if(!ImageIO::loadEXR(a.m_colorImage, value)) { cout << "ERROR in program arguments: couldn't load input color image file '" << value << "'" << endl; return false; }
				missingColor = false;
			}
			else if(flag == "-h")
			{
				Deepimf histAndNbOfSamplesImage;
				if(!ImageIO::loadMultiChannelsEXR(histAndNbOfSamplesImage, value)) { cout << "ERROR in program arguments: couldn't load input histogram image file '" << value << "'" << endl; return false; }
				Utils::separateNbOfSamplesFromHistogram(a.m_histogramImage, a.m_nbOfSamplesImage, histAndNbOfSamplesImage);
				missingHist = false;
			}
			else if(flag == "-c")
			{
				if(!ImageIO::loadMultiChannelsEXR(a.m_covarianceImage, value)) { cout << "ERROR in program arguments: couldn't load input covariance matrix image file '" << value << "'" << endl; return false; }
				missingCov = false;
			}
			else if(flag == "-a")
			{
				PipelineParameters preset;
				preset.m_prefilteringParameters.m_performSpikeRemoval = a.m_prefilterSpikes;
				preset.m_prefilteringParameters.m_spikeRemovalThresholdStDevFactor = a.m_prefilterThresholdStDevFactor;
				preset.m_denoiserParameters.m_nbOfScales = a.m_nbOfScales;
				DenoiserParameters& p = preset.m_denoiserParameters.m_monoscaleParameters;
				p.m_histogramDistanceThreshold = a.m_histogramPatchDistanceThreshold; p.m_patchRadius = a.m_patchRadius;
				p.m_searchWindowRadius = a.m_searchWindowRadius; p.m_minEigenValue = a.m_minEigenValue;
				p.m_useRandomPixelOrder = a.m_useRandomPixelOrder; p.m_markedPixelsSkippingProbability = a.m_markedPixelsSkippingProbability;
				if(!ParametersIO::load(preset, value)) { cout << "ERROR in program arguments: couldn't load the parameters file '" << value << "'" << endl; return false; }
				a.m_prefilterSpikes = preset.m_prefilteringParameters.m_performSpikeRemoval;
				a.m_prefilterThresholdStDevFactor = preset.m_prefilteringParameters.m_spikeRemovalThresholdStDevFactor;
				a.m_nbOfScales = preset.m_denoiserParameters.m_nbOfScales;
				a.m_histogramPatchDistanceThreshold = p.m_histogramDistanceThreshold; a.m_patchRadius = p.m_patchRadius;
				a.m_searchWindowRadius = p.m_searchWindowRadius; a.m_minEigenValue = p.m_minEigenValue;
				a.m_useRandomPixelOrder = p.m_useRandomPixelOrder; a.m_markedPixelsSkippingProbability = p.m_markedPixelsSkippingProbability;
				const InputFileNames& names = preset.m_inputFileNames;
				if(!names.m_colors.empty() && missingColor)
				{
					inputColorFilePath = names.m_colors;
					if(!ImageIO::loadEXR(a.m_colorImage, names.m_colors.c_str())) { cout << "ERROR in program arguments: couldn't load input color image file '" << names.m_colors << "'" << endl; return false; }
					missingColor = false;
				}
				if(!names.m_histograms.empty() && missingHist)
				{
					Deepimf histAndNbOfSamplesImage;
					if(!ImageIO::loadMultiChannelsEXR(histAndNbOfSamplesImage, names.m_histograms.c_str())) { cout << "ERROR in program arguments: couldn't load input histogram image file '" << names.m_histograms << "'" << endl; return false; }
					Utils::separateNbOfSamplesFromHistogram(a.m_histogramImage, a.m_nbOfSamplesImage, histAndNbOfSamplesImage);
					missingHist = false;
				}
				if(!names.m_covariances.empty() && missingCov)
				{
					if(!ImageIO::loadMultiChannelsEXR(a.m_covarianceImage, names.m_covariances.c_str())) { cout << "ERROR in program arguments: couldn't load input covariance matrix image file '" << names.m_covariances << "'" << endl; return false; }
					missingCov = false;
				}
			}
			else if(flag == "-d") { a.m_histogramPatchDistanceThreshold = float(atof(value)); if(a.m_histogramPatchDistanceThreshold <= 0.f) return badValue("-d", "expecting a positive floating number"); }
			else if(flag == "-b") { a.m_searchWindowRadius = atoi(value); if(a.m_searchWindowRadius < 0) return badValue("-b", "expecting a non-negative integer"); }
			else if(flag == "-w") { a.m_patchRadius = atoi(value); if(a.m_patchRadius < 0) return badValue("-w", "expecting a non-negative integer"); }
			else if(flag == "-e") { a.m_minEigenValue = float(atof(value)); if(a.m_minEigenValue <= 0.f) return badValue("-e", "expecting a positive floating number"); }
			else if(flag == "-r") { const int v = atoi(value); if(v != 0 && v != 1) return badValue("-r", "expecting 0 or 1"); a.m_useRandomPixelOrder = v == 1; }
			else if(flag == "-p") { const int v = atoi(value); if(v != 0 && v != 1) return badValue("-p", "expecting 0 or 1"); a.m_prefilterSpikes = v == 1; }
			else if(flag == "--p-factor") { a.m_prefilterThresholdStDevFactor = float(atof(value)); if(a.m_prefilterThresholdStDevFactor <= 0.f) return badValue("--p-factor", "expecting a positive floating number"); }
			else if(flag == "-m") { a.m_markedPixelsSkippingProbability = float(atof(value)); if(a.m_markedPixelsSkippingProbability < 0.f || a.m_markedPixelsSkippingProbability > 1.f) return badValue("-m", "expecting a floating number between 0 and 1"); }
			else if(flag == "-s") { a.m_nbOfScales = atoi(value); if(a.m_nbOfScales <= 0) return badValue("-s", "expecting a positive integer"); }
			else if(flag == "--ncores") { a.m_nbOfCores = atoi(value); }
			else if(flag == "--use-cuda") { a.m_useCuda = atoi(value) == 1; }
			else if(flag == "--seed") { a.m_orderSeed = unsigned(strtoul(value, nullptr, 10)); }
			else if(flag == "--nsamples") { nbOfSamplesArgument = value; }
			else if(flag == "--features")
			{
				a.m_featurePath = value;
				if(!ImageIO::loadMultiChannelsEXR(a.m_featureImage, value)) { cout << "ERROR in program arguments: couldn't load feature image file '" << value << "'" << endl; return false; }
			}
			else if(flag == "--feature-variances")
			{
				a.m_featureVariancePath = value;
				if(!ImageIO::loadMultiChannelsEXR(a.m_featureVarianceImage, value)) { cout << "ERROR in program arguments: couldn't load feature variance image file '" << value << "'" << endl; return false; }
			}
			else if(flag == "--feature-floors")
			{	// "0.01,0.01,1e-4"
				a.m_featureFloors.clear();
				const string list(value);
				size_t pos = 0;
				while(pos <= list.size())
				{
					size_t end = list.find(',', pos);
					if(end == string::npos) end = list.size();
					const string item = list.substr(pos, end - pos);
					char* pEnd = nullptr;
					const float floor = strtof(item.c_str(), &pEnd);
					if(item.empty() || pEnd == item.c_str() || *pEnd != '\0' || !(floor >= 0.f) || std::isinf(floor))
						return badValue("--feature-floors", "expecting a list of finite non-negative floating numbers like 0.01,0.01,1e-4");
					a.m_featureFloors.push_back(floor);
					pos = end + 1;
				}
			}
			else if(flag == "--feature-threshold")
			{
				char* pEnd = nullptr;
				a.m_featureThreshold = strtof(value, &pEnd);
				if(pEnd == value || *pEnd != '\0' || !(a.m_featureThreshold >= 0.f) || std::isinf(a.m_featureThreshold)) return badValue("--feature-threshold", "expecting a finite non-negative floating number");
			}
			else if(flag == "--device") { a.m_devices.assign(1, atoi(value)); }
			else if(flag == "--devices")
			{	// "0-7", "0,1,2", "0-3,6"
				a.m_devices.clear();
				const string list(value);
				size_t pos = 0;
				while(pos < list.size())
				{
					size_t end = list.find(',', pos);
					if(end == string::npos) end = list.size();
					const string item = list.substr(pos, end - pos);
					const size_t dash = item.find('-');
					const int first = atoi(item.substr(0, dash).c_str()), last = dash == string::npos ? first : atoi(item.substr(dash + 1).c_str());
					if(item.empty() || first < 0 || last < first) return badValue("--devices", "expecting a list like 0-7 or 0,2,4");
					for(int d = first; d <= last; ++d) a.m_devices.push_back(d);
					pos = end + 1;
				}
				if(a.m_devices.empty()) return badValue("--devices", "expecting a list like 0-7 or 0,2,4");
			}
			else { cout << "ERROR in program arguments: unknown argument " << flag << endl << endl; printUsage(); return false; }
		}
		if(!a.m_momentSelection && !nbOfSamplesArgument.empty()) { cout << "ERROR in program arguments: --nsamples goes with --moment-selection" << endl; return false; }
		if(a.m_featurePath.empty() && (!a.m_featureVariancePath.empty() || !a.m_featureFloors.empty())) { cout << "ERROR in program arguments: --feature-variances and --feature-floors go with --features" << endl; return false; }
		for(const ProgramArguments::Neighbour& rNb : a.m_neighbours)
		{	// the feature gate covers the frame and every neighbour, or nothing (checked here: nothing has touched a device yet)
			if(!a.m_featurePath.empty() && rNb.m_featurePath.empty())
			{
				cout << "ERROR in program arguments: neighbour '" << rNb.m_colorPath << "' has no --neighbour-features while --features is given: every neighbour needs its feature buffers" << endl;
				return false;
			}
			if(a.m_featurePath.empty() && (!rNb.m_featurePath.empty() || !rNb.m_featureVariancePath.empty()))
			{
				cout << "ERROR in program arguments: neighbour '" << rNb.m_colorPath << "' has --neighbour-features but there is no --features for the frame" << endl;
				return false;
			}
			if(rNb.m_featurePath.empty() && !rNb.m_featureVariancePath.empty())
			{
				cout << "ERROR in program arguments: --neighbour-feature-variances goes with --neighbour-features (neighbour '" << rNb.m_colorPath << "')" << endl;
				return false;
			}
			if(!a.m_featurePath.empty() && a.m_featureVariancePath.empty() != rNb.m_featureVariancePath.empty())
			{
				cout << "ERROR in program arguments: feature variances go with the frame and every neighbour or with none: --feature-variances is "
						<< (a.m_featureVariancePath.empty() ? "absent" : "given") << ", --neighbour-feature-variances of neighbour '" << rNb.m_colorPath << "' is "
						<< (rNb.m_featureVariancePath.empty() ? "absent" : "given") << endl;
				return false;
			}
			for(const Deepimf* pImage : { &rNb.m_featureImage, &rNb.m_featureVarianceImage })
				if(!a.m_featurePath.empty() && (pImage == &rNb.m_featureImage || !rNb.m_featureVariancePath.empty())
						&& (pImage->getWidth() != a.m_featureImage.getWidth() || pImage->getHeight() != a.m_featureImage.getHeight() || pImage->getDepth() != a.m_featureImage.getDepth()))
				{
					cout << "ERROR in program arguments: the feature images of neighbour '" << rNb.m_colorPath << "' must be " << a.m_featureImage.getWidth() << "x" << a.m_featureImage.getHeight()
							<< "x" << a.m_featureImage.getDepth() << " like the --features image (one is " << pImage->getWidth() << "x" << pImage->getHeight() << "x" << pImage->getDepth() << ")" << endl;
					return false;
				}
		}
		if(!a.m_featurePath.empty())
		{	// (checked here: nothing has touched a device yet)
			const int depth = a.m_featureImage.getDepth();
			if(depth < 1 || depth > 8) { cout << "ERROR in program arguments: feature image '" << a.m_featurePath << "' has " << depth << " channels, 1 to 8 are supported" << endl; return false; }
			if(a.m_featureFloors.empty()) { cout << "ERROR in program arguments: --features needs --feature-floors <a,b,...>, one number per feature channel" << endl; return false; }
			if(int(a.m_featureFloors.size()) != depth) { cout << "ERROR in program arguments: " << a.m_featureFloors.size() << " --feature-floors for " << depth << " feature channels" << endl; return false; }
			if(!a.m_featureVariancePath.empty() && (a.m_featureVarianceImage.getWidth() != a.m_featureImage.getWidth() || a.m_featureVarianceImage.getHeight() != a.m_featureImage.getHeight() || a.m_featureVarianceImage.getDepth() != depth))
			{
				cout << "ERROR in program arguments: feature variance image '" << a.m_featureVariancePath << "' is " << a.m_featureVarianceImage.getWidth() << "x" << a.m_featureVarianceImage.getHeight()
						<< "x" << a.m_featureVarianceImage.getDepth() << " but the feature image is " << a.m_featureImage.getWidth() << "x" << a.m_featureImage.getHeight() << "x" << depth << endl;
				return false;
			}
			bool counts = !a.m_featureVariancePath.empty();
			for(float floor : a.m_featureFloors) counts = counts || floor > 0.f;
			if(!counts) { cout << "ERROR in program arguments: every --feature-floors value is 0 and there are no --feature-variances: no feature channel can count" << endl; return false; }
			if(a.m_devices.size() > 1) { cout << "ERROR in program arguments: --features is not available with several devices" << endl; return false; }
			if(!missingColor && (a.m_featureImage.getWidth() != a.m_colorImage.getWidth() || a.m_featureImage.getHeight() != a.m_colorImage.getHeight()))
			{
				cout << "ERROR in program arguments: feature image '" << a.m_featurePath << "' is " << a.m_featureImage.getWidth() << "x" << a.m_featureImage.getHeight()
						<< " but the input color image is " << a.m_colorImage.getWidth() << "x" << a.m_colorImage.getHeight() << endl;
				return false;
			}
		}
		if(!missingColor && inputColorFilePath.length() > 4)
		{
			const string stem = inputColorFilePath.substr(0, inputColorFilePath.length() - 4); // drops ".exr"
			if(missingHist && !a.m_momentSelection)
			{
				const string path = stem + "_hist.exr";
				cout << "Warning: input histogram file not provided by -h argument: assuming '" << path << "'" << endl;
				Deepimf histAndNbOfSamplesImage;
				if(!ImageIO::loadMultiChannelsEXR(histAndNbOfSamplesImage, path.c_str())) { cout << "ERROR in program arguments: couldn't load input histogram image file '" << path << "'" << endl; return false; }
				Utils::separateNbOfSamplesFromHistogram(a.m_histogramImage, a.m_nbOfSamplesImage, histAndNbOfSamplesImage);
				missingHist = false;
			}
			if(missingCov)
			{
				const string path = stem + "_cov.exr";
				cout << "Warning: input covariance file not provided by -c argument: assuming '" << path << "'" << endl;
				if(!ImageIO::loadMultiChannelsEXR(a.m_covarianceImage, path.c_str())) { cout << "ERROR in program arguments: couldn't load input covariance matrix image file '" << path << "'" << endl; return false; }
				missingCov = false;
			}
		}
		if(a.m_momentSelection)
		{	// no histogram: the sample counts come from --nsamples, else from the -h file that was given all the same
			if(!nbOfSamplesArgument.empty() && !missingColor)
			{
				char* pEnd = nullptr;
				const float count = strtof(nbOfSamplesArgument.c_str(), &pEnd);
				if(pEnd != nbOfSamplesArgument.c_str() && *pEnd == '\0')
				{
					if(!(count > 0.f) || std::isinf(count)) return badValue("--nsamples", "expecting a positive number or an EXR file");
					a.m_nbOfSamplesImage.resize(a.m_colorImage.getWidth(), a.m_colorImage.getHeight(), 1);
					a.m_nbOfSamplesImage.fill(count);
				}
				else if(!ImageIO::loadMultiChannelsEXR(a.m_nbOfSamplesImage, nbOfSamplesArgument.c_str()) || a.m_nbOfSamplesImage.getDepth() != 1)
				{
					cout << "ERROR in program arguments: couldn't load a one-channel sample count image from '" << nbOfSamplesArgument << "'" << endl;
					return false;
				}
			}
			else if(missingHist && !missingColor)
			{
				cout << "ERROR in program arguments: --moment-selection needs the sample counts: --nsamples <file|n> (or a -h file)" << endl;
				return false;
			}
			if(a.m_devices.size() > 1) { cout << "ERROR in program arguments: --moment-selection is not available with several devices" << endl; return false; }
			a.m_histogramImage.clearAndFreeMemory();
			missingHist = false;
		}
		for(ProgramArguments::Neighbour& rNb : a.m_neighbours)
		{	// the sample counts (and, without --moment-selection, the histograms) of every neighbour; nothing has touched a device yet
			const string stem = rNb.m_colorPath.substr(0, rNb.m_colorPath.length() - 4);
			if(!a.m_momentSelection)
			{
				if(!rNb.m_nbOfSamplesArgument.empty()) { cout << "ERROR in program arguments: --neighbour-nsamples goes with --moment-selection" << endl; return false; }
				Deepimf histAndNbOfSamplesImage;
				if(!ImageIO::loadMultiChannelsEXR(histAndNbOfSamplesImage, (stem + "_hist.exr").c_str())) { cout << "ERROR in program arguments: couldn't load neighbour histogram image file '" << stem << "_hist.exr'" << endl; return false; }
				Utils::separateNbOfSamplesFromHistogram(rNb.m_histogramImage, rNb.m_nbOfSamplesImage, histAndNbOfSamplesImage);
				continue;
			}
			// --moment-selection: no <frame>_hist.exr is loaded; --neighbour-nsamples of this neighbour, failing that a numeric --nsamples
			char* pEnd = nullptr;
			strtof(nbOfSamplesArgument.c_str(), &pEnd);
			const bool numericFrameCount = !nbOfSamplesArgument.empty() && pEnd != nbOfSamplesArgument.c_str() && *pEnd == '\0';
			const string& rArgument = rNb.m_nbOfSamplesArgument.empty() && numericFrameCount ? nbOfSamplesArgument : rNb.m_nbOfSamplesArgument;
			if(rArgument.empty())
			{
				cout << "ERROR in program arguments: with --moment-selection neighbour '" << rNb.m_colorPath << "' needs its sample counts: --neighbour-nsamples <file|n> after its "
						"--neighbour, or a numeric --nsamples for every frame" << endl;
				return false;
			}
			const float count = strtof(rArgument.c_str(), &pEnd);
			if(pEnd != rArgument.c_str() && *pEnd == '\0')
			{
				if(!(count > 0.f) || std::isinf(count)) return badValue("--neighbour-nsamples", "expecting a positive number or an EXR file");
				rNb.m_nbOfSamplesImage.resize(rNb.m_colorImage.getWidth(), rNb.m_colorImage.getHeight(), 1);
				rNb.m_nbOfSamplesImage.fill(count);
			}
			else if(!ImageIO::loadMultiChannelsEXR(rNb.m_nbOfSamplesImage, rArgument.c_str()) || rNb.m_nbOfSamplesImage.getDepth() != 1)
			{
				cout << "ERROR in program arguments: couldn't load a one-channel sample count image from '" << rArgument << "'" << endl;
				return false;
			}
		}
		if(missingColor || missingHist || missingCov || missingOutput)
		{
			cout << "ERROR: Missing required program argument(s):";
			if(missingColor) cout << " -i";
			if(missingHist) cout << " -h";
			if(missingCov) cout << " -c";
			if(missingOutput) cout << " -o";
			cout << endl << endl;
			printUsage();
			return false;
		}
		// the layers share the geometry of the -i image (checked here: nothing has touched a device yet)
		if(a.m_layers.size() > 15) { cout << "ERROR in program arguments: at most 15 --layer arguments are supported" << endl; return false; }
		for(ProgramArguments::Layer& rLayer : a.m_layers)
		{
			if(rLayer.m_colorImage.getDepth() == 1)
			{	// grey colour file, as for -i
				Deepimf rgb(rLayer.m_colorImage.getWidth(), rLayer.m_colorImage.getHeight(), 3);
				for(int i = 0, n = rLayer.m_colorImage.getSize(); i < n; ++i)
					rgb.get(3 * i) = rgb.get(3 * i + 1) = rgb.get(3 * i + 2) = rLayer.m_colorImage.get(i);
				rLayer.m_colorImage = std::move(rgb);
			}
			const int w = a.m_colorImage.getWidth(), h = a.m_colorImage.getHeight();
			if(rLayer.m_colorImage.getWidth() != w || rLayer.m_colorImage.getHeight() != h || rLayer.m_colorImage.getDepth() != 3)
			{
				cout << "ERROR in program arguments: layer color image '" << rLayer.m_colorPath << "' is " << rLayer.m_colorImage.getWidth() << "x" << rLayer.m_colorImage.getHeight()
						<< "x" << rLayer.m_colorImage.getDepth() << " but the input color image is " << w << "x" << h << endl;
				return false;
			}
			if(rLayer.m_covarianceImage.getWidth() != w || rLayer.m_covarianceImage.getHeight() != h || rLayer.m_covarianceImage.getDepth() != 6)
			{
				cout << "ERROR in program arguments: layer covariance image '" << rLayer.m_covariancePath << "' is " << rLayer.m_covarianceImage.getWidth() << "x"
						<< rLayer.m_covarianceImage.getHeight() << "x" << rLayer.m_covarianceImage.getDepth() << " but " << w << "x" << h << "x6 is expected" << endl;
				return false;
			}
			if(rLayer.m_outputPath == a.m_denoisedOutputFilePath) { cout << "ERROR in program arguments: layer output '" << rLayer.m_outputPath << "' is also the -o output" << endl; return false; }
		}
		if(!a.m_layers.empty() && a.m_prefilterSpikes && !a.m_prefilterLayers && !(a.m_prefilterFrames && !a.m_neighbours.empty())) // (beside neighbours --prefilter-frames covers every layer)
		{
			cout << "ERROR in program arguments: --layer is not available with the spike prefilter (it moves whole pixels by the -i colours): add -p 0, or --prefilter-layers to gather every layer through its decision" << endl;
			return false;
		}
		if(!a.m_layers.empty() && a.m_devices.size() > 1) { cout << "ERROR in program arguments: --layer is not available with several devices" << endl; return false; }
		// every --neighbour brings one --neighbour-layer per --layer, in the size of the -i image (checked here: nothing has touched a device yet)
		for(ProgramArguments::Neighbour& rNb : a.m_neighbours)
		{
			const int w = a.m_colorImage.getWidth(), h = a.m_colorImage.getHeight();
			if(!rNb.m_motionPath.empty() && (rNb.m_motionImage.getWidth() != w || rNb.m_motionImage.getHeight() != h))
			{
				cout << "ERROR in program arguments: neighbour motion image '" << rNb.m_motionPath << "' is not " << w << "x" << h << " like the input color image" << endl;
				return false;
			}
			if(rNb.m_layers.size() != a.m_layers.size())
			{
				cout << "ERROR in program arguments: neighbour '" << rNb.m_colorPath << "' has " << rNb.m_layers.size() << " --neighbour-layer argument(s) but there are "
						<< a.m_layers.size() << " --layer argument(s): every neighbour needs one per layer, in the same order" << endl;
				return false;
			}
			for(ProgramArguments::NeighbourLayer& rLayer : rNb.m_layers)
			{
				if(rLayer.m_colorImage.getDepth() == 1)
				{
					Deepimf rgb(rLayer.m_colorImage.getWidth(), rLayer.m_colorImage.getHeight(), 3);
					for(int i = 0, n = rLayer.m_colorImage.getSize(); i < n; ++i)
						rgb.get(3 * i) = rgb.get(3 * i + 1) = rgb.get(3 * i + 2) = rLayer.m_colorImage.get(i);
					rLayer.m_colorImage = std::move(rgb);
				}
				if(rLayer.m_colorImage.getWidth() != w || rLayer.m_colorImage.getHeight() != h || rLayer.m_colorImage.getDepth() != 3
						|| rLayer.m_covarianceImage.getWidth() != w || rLayer.m_covarianceImage.getHeight() != h || rLayer.m_covarianceImage.getDepth() != 6)
				{
					cout << "ERROR in program arguments: neighbour layer '" << rLayer.m_colorPath << "' / '" << rLayer.m_covariancePath << "' is not " << w << "x" << h
							<< "x3 / " << w << "x" << h << "x6 like the input color image" << endl;
					return false;
				}
			}
		}
		return true;
	}

	// negative, infinite and NaN values are put to zero before writing (src/cli/main.cpp:389-420)
	void checkAndPutToZeroNegativeInfNaNValues(DeepImage<float>& io_rImage)
	{
		float* p = io_rImage.getDataPtr();
		for(int i = 0, n = io_rImage.getSize(); i < n; ++i)
			if(p[i] < 0 || std::isnan(p[i]) || std::isinf(p[i]))
				p[i] = 0.f;
	}

	// "frames/shot.%04d.exr" with one integer conversion and nothing else after a '%'
	bool isFramePattern(const string& i_rPattern)
	{
		const size_t pos = i_rPattern.find('%');
		if(pos == string::npos || i_rPattern.find('%', pos + 1) != string::npos)
			return false;
		size_t i = pos + 1;
		while(i < i_rPattern.size() && isdigit((unsigned char)i_rPattern[i])) ++i;
		return i < i_rPattern.size() && i_rPattern[i] == 'd' && i - pos <= 4;
	}

	string frameName(const string& i_rPattern, int i_frame)
	{
		std::vector<char> buffer(i_rPattern.size() + 32);
		snprintf(buffer.data(), buffer.size(), i_rPattern.c_str(), i_frame);
		return string(buffer.data());
	}

	// --sequence-in: the frames --first .. --last through bcd::SequenceDenoiser.  Everything is checked before the first file is read or a device is asked for
	int launchSequenceDenoising(int argc, const char** argv)
	{
		ProgramArguments a;
		a.m_prefilterSpikes = true; // (the CLI's default: the sequence takes the prefilter through --prefilter-frames only, else -p 0 must be said)
		string inPattern, outPattern;
		int first = 0, last = -1, radius = 1;
		bool hasFirst = false, hasLast = false;
		// colour layers, the moment selection and the feature gate of a sequence: file patterns per frame (SequenceDenoiser::setFrameSettings)
		struct SequenceLayer { string m_colorPattern, m_covariancePattern, m_outputPattern; };
		std::vector<SequenceLayer> layers;
		bool moments = false;
		float momentFloor = 1e-8f, featureThreshold = 1.f;
		string nbOfSamplesPattern, featurePattern, featureVariancePattern;
		string motionPattern[2]; // --sequence-motion-prev, --sequence-motion-next
		std::vector<float> featureFloors;
		auto argumentError = [](const string& i_rMessage) { cout << "ERROR in program arguments: " << i_rMessage << endl; return 1; };
		for(int i = 1; i < argc; ++i)
		{
			const string flag = argv[i];
			if(flag == "--help") { printUsage(); return 1; }
			if(flag == "--prefilter-frames") { a.m_prefilterFrames = true; continue; }
			for(const char* pOther : { "-i", "-o", "-h", "-c", "-a", "--neighbour", "--neighbour-nsamples", "--neighbour-motion", "--neighbour-features", "--neighbour-feature-variances",
					"--neighbour-layer", "--layer", "--prefilter-layers", "--moment-selection", "--nsamples", "--features", "--feature-variances", "--feature-floors",
					"--feature-threshold", "--devices" })
				if(flag == pOther)
					return argumentError(flag + " is not available with --sequence-in (a sequence reads <frame>.exr, <frame>_hist.exr and <frame>_cov.exr of every frame and writes "
							"--sequence-out; one colour layer, histogram selection, one device)");
			if(i + 1 >= argc) return argumentError("expecting a value after " + flag);
			if(flag == "--sequence-layer")
			{	// one further colour layer of every frame: its colours, its covariances, its output -- three patterns with the frame number
				if(i + 3 >= argc) return argumentError("expecting <colour pattern> <covariance pattern> <output pattern> after --sequence-layer");
				SequenceLayer layer = { argv[i + 1], argv[i + 2], argv[i + 3] };
				if(!isFramePattern(layer.m_colorPattern) || !isFramePattern(layer.m_covariancePattern) || !isFramePattern(layer.m_outputPattern))
					return argumentError("--sequence-layer needs three file patterns with one %d each: colours, covariances, output");
				if(layer.m_outputPattern == layer.m_colorPattern || layer.m_outputPattern == layer.m_covariancePattern)
					return argumentError("the output of a --sequence-layer would overwrite its input");
				layers.push_back(layer);
				i += 3;
				continue;
			}
			const char* value = argv[++i];
			if(flag == "--sequence-moments")
			{	// the selection from means and covariances: the variance floor; the sample counts come from --sequence-nsamples, no <frame>_hist.exr is read
				char* pEnd = nullptr;
				momentFloor = strtof(value, &pEnd);
				if(pEnd == value || *pEnd || !(momentFloor >= 0.f) || std::isinf(momentFloor)) return argumentError("expecting a finite non-negative variance floor after --sequence-moments");
				moments = true;
			}
			else if(flag == "--sequence-nsamples") nbOfSamplesPattern = value;
			else if(flag == "--sequence-features") featurePattern = value;
			else if(flag == "--sequence-feature-variances") featureVariancePattern = value;
			else if(flag == "--sequence-feature-floors")
			{	// "0.01,0.01,1e-4", as --feature-floors
				featureFloors.clear();
				const string list(value);
				for(size_t pos = 0; pos <= list.size();)
				{
					size_t end = list.find(',', pos);
					if(end == string::npos) end = list.size();
					const string item = list.substr(pos, end - pos);
					char* pEnd = nullptr;
					const float floor = strtof(item.c_str(), &pEnd);
					if(item.empty() || *pEnd || !(floor >= 0.f) || std::isinf(floor))
						return argumentError("expecting a list of finite non-negative floating numbers like 0.01,0.01,1e-4 after --sequence-feature-floors");
					featureFloors.push_back(floor);
					pos = end + 1;
				}
			}
			else if(flag == "--sequence-feature-threshold")
			{
				char* pEnd = nullptr;
				featureThreshold = strtof(value, &pEnd);
				if(pEnd == value || *pEnd || !(featureThreshold >= 0.f) || std::isinf(featureThreshold)) return argumentError("expecting a finite non-negative number after --sequence-feature-threshold");
			}
			else if(flag == "--sequence-motion-prev") motionPattern[0] = value;
			else if(flag == "--sequence-motion-next") motionPattern[1] = value;
			else if(flag == "--sequence-in") inPattern = value;
			else if(flag == "--sequence-out") outPattern = value;
			else if(flag == "--first") { first = atoi(value); hasFirst = true; }
			else if(flag == "--last") { last = atoi(value); hasLast = true; }
			else if(flag == "--temporal-radius") radius = atoi(value);
			else if(flag == "-d") { a.m_histogramPatchDistanceThreshold = float(atof(value)); if(a.m_histogramPatchDistanceThreshold <= 0.f) return argumentError(string("expecting a positive floating number") + " after " + "-d"); }
			else if(flag == "-b") a.m_searchWindowRadius = atoi(value);
			else if(flag == "-w") a.m_patchRadius = atoi(value);
			else if(flag == "-e") { a.m_minEigenValue = float(atof(value)); if(a.m_minEigenValue <= 0.f) return argumentError(string("expecting a positive floating number") + " after " + "-e"); }
			else if(flag == "-r") { const int v = atoi(value); if(v != 0 && v != 1) return argumentError(string("expecting 0 or 1") + " after " + "-r"); a.m_useRandomPixelOrder = v == 1; }
			else if(flag == "-p") { const int v = atoi(value); if(v != 0 && v != 1) return argumentError(string("expecting 0 or 1") + " after " + "-p"); a.m_prefilterSpikes = v == 1; }
			else if(flag == "-m") { a.m_markedPixelsSkippingProbability = float(atof(value)); if(a.m_markedPixelsSkippingProbability < 0.f || a.m_markedPixelsSkippingProbability > 1.f) return argumentError(string("expecting a floating number between 0 and 1") + " after " + "-m"); }
			else if(flag == "-s") { a.m_nbOfScales = atoi(value); if(a.m_nbOfScales <= 0) return argumentError(string("expecting a positive integer") + " after " + "-s"); }
			else if(flag == "--ncores") a.m_nbOfCores = atoi(value);
			else if(flag == "--use-cuda") a.m_useCuda = atoi(value) == 1;
			else if(flag == "--seed") a.m_orderSeed = unsigned(strtoul(value, nullptr, 10));
			else if(flag == "--device") a.m_devices.assign(1, atoi(value));
			else if(flag == "--p-factor") { const float v = float(atof(value)); if(v > 0.f) a.m_prefilterThresholdStDevFactor = v; } // (read by --prefilter-frames)
			else return argumentError("unknown argument " + flag + " (beside --sequence-in)");
		}
		if(!isFramePattern(inPattern)) return argumentError("--sequence-in needs a file pattern with one %d for the frame number, like frames/shot.%04d.exr");
		if(!isFramePattern(outPattern)) return argumentError("--sequence-out <pattern with %d> is required beside --sequence-in");
		if(inPattern == outPattern) return argumentError("--sequence-out would overwrite the --sequence-in frames");
		if(!hasFirst || !hasLast || first < 0 || last < first) return argumentError("--first <a> and --last <b> with 0 <= a <= b are required beside --sequence-in");
		if(radius < 1 || radius > 2) return argumentError("--temporal-radius must be 1 or 2");
		if(a.m_prefilterSpikes && !a.m_prefilterFrames) return argumentError("--sequence-in is not available with the spike prefilter: add -p 0, or --prefilter-frames");
		if(a.m_patchRadius != 1 || a.m_searchWindowRadius != 6) return argumentError("--sequence-in needs -w 1 and -b 6 (neighbour frames support no other geometry)");
		if(frameName(inPattern, first).length() <= 4) return argumentError("'" + frameName(inPattern, first) + "' is no .exr file name");
		if(layers.size() > 15) return argumentError("at most 15 --sequence-layer arguments");
		for(const SequenceLayer& rLayer : layers)
			if(rLayer.m_outputPattern == inPattern || rLayer.m_outputPattern == outPattern) return argumentError("the output of a --sequence-layer would overwrite another file of the sequence");
		if(moments && !isFramePattern(nbOfSamplesPattern)) return argumentError("--sequence-moments needs --sequence-nsamples <pattern with %d>: the sample counts of every frame (no <frame>_hist.exr is read)");
		if(!moments && !nbOfSamplesPattern.empty()) return argumentError("--sequence-nsamples goes with --sequence-moments");
		if(featurePattern.empty() && (!featureVariancePattern.empty() || !featureFloors.empty())) return argumentError("--sequence-feature-variances and --sequence-feature-floors go with --sequence-features");
		if(!featurePattern.empty())
		{
			if(!isFramePattern(featurePattern) || (!featureVariancePattern.empty() && !isFramePattern(featureVariancePattern)))
				return argumentError("--sequence-features and --sequence-feature-variances need a file pattern with one %d");
			if(featureFloors.empty() || featureFloors.size() > 8) return argumentError("--sequence-features needs --sequence-feature-floors <a,b,...>, one number per feature channel (1 to 8)");
			bool counts = !featureVariancePattern.empty();
			for(float floor : featureFloors) counts = counts || floor > 0.f;
			if(!counts) return argumentError("every --sequence-feature-floors value is 0 and there are no --sequence-feature-variances: no feature channel can count");
		}
		for(const string& rPattern : motionPattern)
			if(!rPattern.empty() && !isFramePattern(rPattern))
				return argumentError("--sequence-motion-prev and --sequence-motion-next need a file pattern with one %d for the frame number");
		const bool frameSettings = !layers.empty() || moments || !featurePattern.empty();

		DenoiserParameters parameters;
		parameters.m_histogramDistanceThreshold = a.m_histogramPatchDistanceThreshold;
		parameters.m_patchRadius = a.m_patchRadius;
		parameters.m_searchWindowRadius = a.m_searchWindowRadius;
		parameters.m_minEigenValue = a.m_minEigenValue;
		parameters.m_useRandomPixelOrder = a.m_useRandomPixelOrder;
		parameters.m_markedPixelsSkippingProbability = a.m_markedPixelsSkippingProbability;
		parameters.m_nbOfCores = a.m_nbOfCores;
		parameters.m_useCuda = a.m_useCuda;
		SequenceDenoiser sequence(a.m_nbOfScales, radius);
		sequence.setParameters(parameters);
		sequence.setOrderSeed(a.m_orderSeed);
		sequence.setDevices(a.m_devices);
		sequence.setZeroBadOutputValues(true);
		sequence.setFrameSettings(frameSettings);
		if(a.m_prefilterSpikes && a.m_prefilterFrames)
		{	// every pushed frame is prefiltered once, in place in its slot
			sequence.setSpikePrefilterFrames(true);
			sequence.setSpikePrefilter(a.m_prefilterThresholdStDevFactor);
		}
		if(moments) sequence.setMomentSelection(true, momentFloor);
		if(!sequence.settingsAreOk())
			return 1;
		std::vector<Deepimf> layerOutputs(layers.size());
		auto popReady = [&]() -> int
		{
			while(sequence.ready() > 0)
			{
				Deepimf out;
				DenoiserOutputs outputs;
				outputs.m_pDenoisedColors = &out;
				sequence.clearLayers(); // (a pop writes the layers registered now: only their outputs are looked at)
				for(Deepimf& rOut : layerOutputs) sequence.addLayer(nullptr, nullptr, &rOut);
				if(!sequence.popFrame(outputs))
					return 2;
				for(size_t k = 0; k < layers.size(); ++k)
				{
					checkAndPutToZeroNegativeInfNaNValues(layerOutputs[k]);
					const string layerPath = frameName(layers[k].m_outputPattern, first + int(sequence.getLastFrameIndex()));
					if(!ImageIO::writeEXR(layerOutputs[k], layerPath.c_str()))
					{
						cerr << "Couldn't write " << layerPath << ": " << ImageIO::lastError() << endl;
						return 3;
					}
				}
				checkAndPutToZeroNegativeInfNaNValues(out);
				const string path = frameName(outPattern, first + int(sequence.getLastFrameIndex()));
				if(!ImageIO::writeEXR(out, path.c_str()))
				{
					cerr << "Couldn't write " << path << ": " << ImageIO::lastError() << endl;
					return 3;
				}
				cout << "Written denoised frame " << first + sequence.getLastFrameIndex() << " in file " << path << endl;
			}
			return 0;
		};
		for(int frame = first; frame <= last; ++frame)
		{
			const string path = frameName(inPattern, frame), stem = path.substr(0, path.length() - 4);
			Deepimf color, histAndNbOfSamples, hist, nbOfSamples, cov;
			if(!ImageIO::loadEXR(color, path.c_str())) return argumentError("couldn't load input color image file '" + path + "'");
			if(moments)
			{
				const string nsPath = frameName(nbOfSamplesPattern, frame);
				if(!ImageIO::loadMultiChannelsEXR(nbOfSamples, nsPath.c_str()) || nbOfSamples.getDepth() != 1) return argumentError("couldn't load a one-channel sample count image from '" + nsPath + "'");
			}
			else if(!ImageIO::loadMultiChannelsEXR(histAndNbOfSamples, (stem + "_hist.exr").c_str())) return argumentError("couldn't load input histogram image file '" + stem + "_hist.exr'");
			if(!ImageIO::loadMultiChannelsEXR(cov, (stem + "_cov.exr").c_str())) return argumentError("couldn't load input covariance matrix image file '" + stem + "_cov.exr'");
			if(!moments) Utils::separateNbOfSamplesFromHistogram(hist, nbOfSamples, histAndNbOfSamples);
			// the frame's further layers and feature buffers: registered for this push (the class checks their sizes against the frame)
			std::vector<Deepimf> layerColors(layers.size()), layerCovariances(layers.size());
			Deepimf features, featureVariances;
			sequence.clearLayers();
			for(size_t k = 0; k < layers.size(); ++k)
			{
				const string colorPath = frameName(layers[k].m_colorPattern, frame), covariancePath = frameName(layers[k].m_covariancePattern, frame);
				if(!ImageIO::loadEXR(layerColors[k], colorPath.c_str())) return argumentError("couldn't load layer color image file '" + colorPath + "'");
				if(!ImageIO::loadMultiChannelsEXR(layerCovariances[k], covariancePath.c_str())) return argumentError("couldn't load layer covariance image file '" + covariancePath + "'");
				sequence.addLayer(&layerColors[k], &layerCovariances[k], &layerOutputs[k]);
			}
			if(!featurePattern.empty())
			{
				const string featurePath = frameName(featurePattern, frame);
				if(!ImageIO::loadMultiChannelsEXR(features, featurePath.c_str())) return argumentError("couldn't load feature image file '" + featurePath + "'");
				if(!featureVariancePattern.empty() && !ImageIO::loadMultiChannelsEXR(featureVariances, frameName(featureVariancePattern, frame).c_str()))
					return argumentError("couldn't load feature variance image file '" + frameName(featureVariancePattern, frame) + "'");
				if(features.getDepth() != int(featureFloors.size()))
					return argumentError(std::to_string(featureFloors.size()) + " --sequence-feature-floors for " + std::to_string(features.getDepth()) + " feature channels of '" + featurePath + "'");
				sequence.setGuideFeatures(&features, featureVariancePattern.empty() ? nullptr : &featureVariances, featureFloors, featureThreshold);
			}
			if(color.getDepth() == 1)
			{	// grey colour file, as for -i
				Deepimf rgb(color.getWidth(), color.getHeight(), 3);
				for(int i = 0, n = color.getSize(); i < n; ++i)
					rgb.get(3 * i) = rgb.get(3 * i + 1) = rgb.get(3 * i + 2) = color.get(i);
				color = std::move(rgb);
			}
			// the frame's motion fields, (dx, dy) in the first two channels; the first frame has no frame before it and the last none after it: their files may be missing
			Deepimf motion[2];
			for(int d = 0; d < 2; ++d)
			{
				if(motionPattern[d].empty()) continue;
				const string motionPath = frameName(motionPattern[d], frame);
				if(frame == (d ? last : first) && !std::ifstream(motionPath.c_str()).good()) continue;
				Deepimf loaded;
				if(!ImageIO::loadMultiChannelsEXR(loaded, motionPath.c_str())) return argumentError("couldn't load motion image file '" + motionPath + "'");
				if(loaded.getDepth() < 2) return argumentError("motion image '" + motionPath + "' needs two channels (dx, dy)");
				motion[d].resize(loaded.getWidth(), loaded.getHeight(), 2);
				const int depth = loaded.getDepth();
				for(size_t px = 0, n = size_t(loaded.getWidth()) * loaded.getHeight(); px < n; ++px)
				{
					motion[d].get(int(2 * px)) = loaded.get(int(depth * px));
					motion[d].get(int(2 * px + 1)) = loaded.get(int(depth * px + 1));
				}
			}
			sequence.setFrameMotion(motion[0].isEmpty() ? nullptr : &motion[0], motion[1].isEmpty() ? nullptr : &motion[1]);
			DenoiserInputs inputs;
			inputs.m_pColors = &color; inputs.m_pNbOfSamples = &nbOfSamples; inputs.m_pHistograms = moments ? nullptr : &hist; inputs.m_pSampleCovariances = &cov;
			if(!sequence.pushFrame(inputs))
				return 2;
			sequence.setGuideFeatures(nullptr, nullptr, featureFloors, featureThreshold); // (the frame's images end with this iteration)
			if(frame == last && !sequence.end())
				return 2;
			const int rc = popReady();
			if(rc != 0)
				return rc;
		}
		return 0;
	}

	int launchBayesianCollaborativeDenoising(int argc, const char** argv)
	{
		// --use-cuda 0 asks for the reference's CPU/OpenMP loop, which this build does not have (one product path: the HIP device).  The library
		// declines the request with a note and runs on the device (Denoiser.cpp); under BCD_STRICT_CPU_REQUEST=1 it refuses instead, and that is
		// said here, before the input files are read, not after minutes of EXR decoding
		{
			const char* pStrict = getenv("BCD_STRICT_CPU_REQUEST");
			for(int i = 1; i + 1 < argc; ++i)
				if(string(argv[i]) == "--use-cuda" && atoi(argv[i + 1]) != 1 && pStrict != nullptr && pStrict[0] == '1')
				{
					cerr << "bcd_cli: --use-cuda 0 requests the CPU/OpenMP path, which this build does not have, and BCD_STRICT_CPU_REQUEST=1 forbids "
							"answering it with the HIP device; nothing was read or written" << endl;
					return 2;
				}
		}
		bool sequenceIn = false, sequenceOut = false, sequenceMotion = false;
		for(int i = 1; i < argc; ++i)
		{
			sequenceIn = sequenceIn || string(argv[i]) == "--sequence-in";
			sequenceOut = sequenceOut || string(argv[i]) == "--sequence-out";
			sequenceMotion = sequenceMotion || string(argv[i]) == "--sequence-motion-prev" || string(argv[i]) == "--sequence-motion-next";
		}
		if(sequenceMotion && !sequenceIn)
		{
			cout << "ERROR in program arguments: --sequence-motion-prev and --sequence-motion-next go with --sequence-in (beside -i a neighbour's field is --neighbour-motion)" << endl;
			return 1;
		}
		if(sequenceIn || sequenceOut)
			return launchSequenceDenoising(argc, argv);
		ProgramArguments args;
		if(!parseProgramArguments(argc, argv, args))
			return 1;
		if(args.m_colorImage.getDepth() == 1)
		{	// grey colour file: the denoiser works on 3 channels
			Deepimf rgb(args.m_colorImage.getWidth(), args.m_colorImage.getHeight(), 3);
			for(int i = 0, n = args.m_colorImage.getSize(); i < n; ++i)
				rgb.get(3 * i) = rgb.get(3 * i + 1) = rgb.get(3 * i + 2) = args.m_colorImage.get(i);
			args.m_colorImage = std::move(rgb);
		}
		// -p 1 (src/cli/main.cpp:428-441): on one device the prefilter runs on the uploaded copies, right before the denoiser (one trip
		// over PCIe for everything); with several devices it runs first, as in the reference
		const bool prefilterOnDevice = args.m_prefilterSpikes && args.m_devices.size() == 1;
		if(args.m_prefilterSpikes && !prefilterOnDevice)
			SpikeRemovalFilter::filter(args.m_colorImage, args.m_nbOfSamplesImage, args.m_histogramImage, args.m_covarianceImage, args.m_prefilterThresholdStDevFactor);

		DenoiserInputs inputs;
		inputs.m_pColors = &args.m_colorImage;
		inputs.m_pNbOfSamples = &args.m_nbOfSamplesImage;
		inputs.m_pHistograms = args.m_momentSelection ? nullptr : &args.m_histogramImage;
		inputs.m_pSampleCovariances = &args.m_covarianceImage;
		Deepimf outputDenoisedColorImage(args.m_colorImage);
		DenoiserOutputs outputs;
		outputs.m_pDenoisedColors = &outputDenoisedColorImage;
		DenoiserParameters parameters;
		parameters.m_histogramDistanceThreshold = args.m_histogramPatchDistanceThreshold;
		parameters.m_patchRadius = args.m_patchRadius;
		parameters.m_searchWindowRadius = args.m_searchWindowRadius;
		parameters.m_minEigenValue = args.m_minEigenValue;
		parameters.m_useRandomPixelOrder = args.m_useRandomPixelOrder;
		parameters.m_markedPixelsSkippingProbability = args.m_markedPixelsSkippingProbability;
		parameters.m_nbOfCores = args.m_nbOfCores;
		parameters.m_useCuda = args.m_useCuda;

		unique_ptr<IDenoiser> uDenoiser;
		HipEngineSettings* pSettings = nullptr;
		if(args.m_nbOfScales > 1) { MultiscaleDenoiser* p = new MultiscaleDenoiser(args.m_nbOfScales); uDenoiser.reset(p); pSettings = p; }
		else { Denoiser* p = new Denoiser(); uDenoiser.reset(p); pSettings = p; }
		pSettings->setOrderSeed(args.m_orderSeed);
		pSettings->setDevices(args.m_devices);
		if(prefilterOnDevice)
			pSettings->setSpikePrefilter(args.m_prefilterThresholdStDevFactor);
		pSettings->setSpikePrefilterLayers(args.m_prefilterLayers);
		pSettings->setSpikePrefilterFrames(args.m_prefilterFrames);
		pSettings->setMomentSelection(args.m_momentSelection, args.m_momentVarianceFloor);
		if(!args.m_featurePath.empty())
			pSettings->setGuideFeatures(&args.m_featureImage, args.m_featureVariancePath.empty() ? nullptr : &args.m_featureVarianceImage, args.m_featureFloors, args.m_featureThreshold);
		pSettings->setZeroBadOutputValues(true); // checkAndPutToZeroNegativeInfNaNValues (src/cli/main.cpp:470) before the download
		for(ProgramArguments::Neighbour& rNb : args.m_neighbours)
		{
			DenoiserInputs frame;
			frame.m_pColors = &rNb.m_colorImage; frame.m_pNbOfSamples = &rNb.m_nbOfSamplesImage; frame.m_pSampleCovariances = &rNb.m_covarianceImage;
			frame.m_pHistograms = args.m_momentSelection ? nullptr : &rNb.m_histogramImage;
			if(args.m_momentSelection)
				pSettings->addNeighbourFrameMoments(frame);
			else
				pSettings->addNeighbourFrame(frame);
			for(ProgramArguments::NeighbourLayer& rLayer : rNb.m_layers)
				pSettings->addNeighbourFrameLayer(pSettings->getNeighbourFrames().size() - 1, &rLayer.m_colorImage, &rLayer.m_covarianceImage);
			if(!rNb.m_motionPath.empty())
				pSettings->setNeighbourMotion(pSettings->getNeighbourFrames().size() - 1, &rNb.m_motionImage);
			if(!rNb.m_featurePath.empty())
				pSettings->setNeighbourGuideFeatures(pSettings->getNeighbourFrames().size() - 1, &rNb.m_featureImage, rNb.m_featureVariancePath.empty() ? nullptr : &rNb.m_featureVarianceImage);
		}
		std::vector<Deepimf> layerOutputs(args.m_layers.size());
		for(size_t k = 0; k < args.m_layers.size(); ++k)
			pSettings->addLayer(&args.m_layers[k].m_colorImage, &args.m_layers[k].m_covarianceImage, &layerOutputs[k]);
		uDenoiser->setInputs(inputs);
		uDenoiser->setOutputs(outputs);
		uDenoiser->setParameters(parameters);
		if(!uDenoiser->denoise())
			return 2;

		checkAndPutToZeroNegativeInfNaNValues(outputDenoisedColorImage); // (already clean: kept as the reference's last line of defence)
		if(!ImageIO::writeEXR(outputDenoisedColorImage, args.m_denoisedOutputFilePath.c_str()))
		{
			cerr << "Couldn't write " << args.m_denoisedOutputFilePath << ": " << ImageIO::lastError() << endl;
			return 3;
		}
		cout << "Written denoised output in file " << args.m_denoisedOutputFilePath << endl;
		for(size_t k = 0; k < args.m_layers.size(); ++k)
		{	// the same last line of defence and the same writer as the main output
			checkAndPutToZeroNegativeInfNaNValues(layerOutputs[k]);
			if(!ImageIO::writeEXR(layerOutputs[k], args.m_layers[k].m_outputPath.c_str()))
			{
				cerr << "Couldn't write " << args.m_layers[k].m_outputPath << ": " << ImageIO::lastError() << endl;
				return 3;
			}
			cout << "Written denoised layer " << k + 1 << " in file " << args.m_layers[k].m_outputPath << endl;
		}
		return 0;
	}

}

int main(int argc, const char** argv)
{
	Chronometer programTotalTime;
	programTotalTime.start();
	g_pProgramPath = argv[0];
	const int rc = launchBayesianCollaborativeDenoising(argc, argv);
	programTotalTime.stop();
	cout << "Program total time: ";
	programTotalTime.printElapsedTime();
	cout << endl;
	return rc;
}
