// SequenceDenoiser.cpp -- bcd::SequenceDenoiser of the MI355X build: the checks that need no device, with messages on cerr in the style of
// Denoiser.cpp, then the host push and pop of the sequence object of the C ABI (bcd_hip_sequence_*, include/bcd_hip.h).  The object owns its engine
// context: the frames it keeps on the device live and die with it.
#include "SequenceDenoiser.h"

#include "DeepImage.h"
#include "bcd_hip.h"

#include <algorithm>
#include <iostream>
#include <limits>
#include <omp.h>

using namespace std;

namespace bcd
{

	SequenceDenoiser::SequenceDenoiser(int i_nbOfScales, int i_temporalRadius) :
			m_nbOfScales(i_nbOfScales), m_temporalRadius(i_temporalRadius), m_pCtx(nullptr), m_pSequence(nullptr), m_width(0), m_height(0), m_depth(0),
			m_lastFrameIndex(-1)
	{
	}

	SequenceDenoiser::~SequenceDenoiser() { release(); }

	void SequenceDenoiser::release()
	{
		if(m_pSequence) bcd_hip_sequence_destroy(m_pSequence); // (before its context)
		if(m_pCtx) bcd_hip_ctx_destroy(static_cast<bcd_hip_ctx*>(m_pCtx));
		m_pSequence = nullptr;
		m_pCtx = nullptr;
	}

	void SequenceDenoiser::reset()
	{
		// (the sequence is created again by the next push: its size, scales, radius and parameters may have changed)
		if(m_pSequence) bcd_hip_sequence_destroy(m_pSequence);
		m_pSequence = nullptr;
		m_lastFrameIndex = -1;
	}

	bool SequenceDenoiser::settingsAreOk() const
	{
		if(m_temporalRadius < 1 || 2 * m_temporalRadius > BCD_HIP_MAX_NEIGHBOURS)
		{
			cerr << "Aborting denoising: the temporal radius of a sequence must be 1 or 2, not " << m_temporalRadius << endl;
			return false;
		}
		if(m_nbOfScales < 1)
		{
			cerr << "Aborting denoising: the number of scales must be at least 1" << endl;
			return false;
		}
		if(m_parameters.m_patchRadius != 1 || m_parameters.m_searchWindowRadius != 6)
		{
			cerr << "Aborting denoising: a sequence is denoised with patch radius 1 and search radius 6 (neighbour frames support no other geometry)" << endl;
			return false;
		}
		if(m_devices.size() > 1)
		{
			cerr << "Aborting denoising: a sequence is not available over several devices" << endl;
			return false;
		}
		if(!m_layers.empty() || !m_neighbourFrames.empty() || m_momentSelection || m_pGuideFeatures || m_prefilterThresholdStDevFactor > 0.f)
		{
			cerr << "Aborting denoising: a sequence takes no added colour layers, no neighbour frames of its own (the window supplies them), no moment selection, no "
					"feature buffers and no spike prefilter" << endl;
			return false;
		}
		return true;
	}

	bool SequenceDenoiser::frameIsOk(const DenoiserInputs& i_rFrame) const
	{
		const DeepImage<float>* images[4] = { i_rFrame.m_pColors, i_rFrame.m_pNbOfSamples, i_rFrame.m_pHistograms, i_rFrame.m_pSampleCovariances };
		const char* names[4] = { "color", "number of samples", "histogram", "covariance" };
		for(int i = 0; i < 4; ++i)
			if(!images[i] || images[i]->isEmpty())
			{
				cerr << "Aborting denoising: nullptr or empty input " << names[i] << " image" << endl;
				return false;
			}
		const int w = images[0]->getWidth(), h = images[0]->getHeight();
		for(int i = 1; i < 4; ++i)
			if(images[i]->getWidth() != w || images[i]->getHeight() != h)
			{
				cerr << "Aborting denoising: input " << names[i] << " image is " << images[i]->getWidth() << "x" << images[i]->getHeight()
						<< " but input color image is " << w << "x" << h << endl;
				return false;
			}
		if(images[0]->getDepth() != 3 || images[1]->getDepth() != 1 || images[3]->getDepth() != 6)
		{
			cerr << "Aborting denoising: expected depths 3 / 1 / 6 for color / number of samples / covariance images" << endl;
			return false;
		}
		if(m_pSequence && (w != m_width || h != m_height || images[2]->getDepth() != m_depth))
		{
			cerr << "Aborting denoising: every frame of a sequence has the size of its first frame (" << m_width << "x" << m_height << ", " << m_depth
					<< " histogram channels)" << endl;
			return false;
		}
		return true;
	}

	bool SequenceDenoiser::pushFrame(const DenoiserInputs& i_rFrame)
	{
		if(!settingsAreOk() || !frameIsOk(i_rFrame))
			return false;
		if(!m_pSequence)
		{
			const int w = i_rFrame.m_pColors->getWidth(), h = i_rFrame.m_pColors->getHeight(), depth = i_rFrame.m_pHistograms->getDepth();
			for(int s = 1, ws = w, hs = h; s < m_nbOfScales; ++s)
			{
				ws /= 2; hs /= 2;
				if(ws < 3 || hs < 3)
				{
					cerr << "Aborting denoising: too many scales for this image size" << endl;
					return false;
				}
			}
			bcd_hip_params prm;
			bcd_hip_default_params(&prm);
			prm.hist_dist_threshold = m_parameters.m_histogramDistanceThreshold;
			prm.patch_radius = m_parameters.m_patchRadius;
			prm.search_radius = m_parameters.m_searchWindowRadius;
			prm.min_eigen_value = m_parameters.m_minEigenValue;
			// the visiting order of Denoiser::denoiseWithNbOfScales: a shuffle (-r 1), else -- more than one thread -- the strip list, else scanline
			const int nbOfCores = m_parameters.m_nbOfCores > 0 ? m_parameters.m_nbOfCores : std::max(1, omp_get_max_threads());
			prm.use_random_pixel_order = m_parameters.m_useRandomPixelOrder ? 1 : (nbOfCores > 1 && w <= 8191 && h <= 8191 ? 2 : 0);
			prm.marked_skip_probability = m_parameters.m_markedPixelsSkippingProbability;
			prm.order_seed = m_orderSeed;
			bcd_hip_ctx* pCtx = static_cast<bcd_hip_ctx*>(m_pCtx);
			if(!pCtx && bcd_hip_ctx_create(&pCtx, m_devices[0], nullptr) != BCD_HIP_OK)
			{
				cerr << "Aborting denoising: no usable HIP device " << m_devices[0] << " (this build has no CPU path)" << endl;
				return false;
			}
			m_pCtx = pCtx;
			if(bcd_hip_sequence_create(pCtx, w, h, depth, m_nbOfScales, m_temporalRadius, &prm, &m_pSequence) != BCD_HIP_OK)
			{
				cerr << "Aborting denoising: " << bcd_hip_last_error(pCtx) << endl;
				m_pSequence = nullptr;
				return false;
			}
			m_width = w; m_height = h; m_depth = depth;
			m_lastFrameIndex = -1;
		}
		if(bcd_hip_sequence_push_host(m_pSequence, i_rFrame.m_pColors->getDataPtr(), i_rFrame.m_pNbOfSamples->getDataPtr(), i_rFrame.m_pHistograms->getDataPtr(),
				i_rFrame.m_pSampleCovariances->getDataPtr()) != BCD_HIP_OK)
		{
			cerr << "Aborting denoising: " << bcd_hip_last_error(static_cast<bcd_hip_ctx*>(m_pCtx)) << endl;
			return false;
		}
		return true;
	}

	bool SequenceDenoiser::end()
	{
		if(!m_pSequence)
		{
			cerr << "Aborting denoising: no frame has been pushed" << endl;
			return false;
		}
		return bcd_hip_sequence_end(m_pSequence) == BCD_HIP_OK;
	}

	int SequenceDenoiser::ready() const { return m_pSequence ? bcd_hip_sequence_ready(m_pSequence) : 0; }

	bool SequenceDenoiser::popFrame(DenoiserOutputs& o_rOutputs)
	{
		if(!o_rOutputs.m_pDenoisedColors)
		{
			cerr << "Aborting denoising: nullptr for output image" << endl;
			return false;
		}
		if(ready() < 1)
		{
			cerr << "Aborting denoising: no frame of the sequence is ready (push its later neighbours, or call end())" << endl;
			return false;
		}
		Deepimf result(m_width, m_height, 3);
		int64_t index = -1;
		if(bcd_hip_sequence_pop_host(m_pSequence, result.getDataPtr(), &index) != BCD_HIP_OK)
		{
			cerr << "Aborting denoising: " << bcd_hip_last_error(static_cast<bcd_hip_ctx*>(m_pCtx)) << endl;
			return false;
		}
		if(m_zeroBadOutputValues)
		{
			float* p = result.getDataPtr();
			for(size_t i = 0, n = size_t(m_width) * m_height * 3; i < n; ++i)
				if(!(p[i] >= 0.f) || !(p[i] <= std::numeric_limits<float>::max()))
					p[i] = 0.f;
		}
		*o_rOutputs.m_pDenoisedColors = std::move(result);
		m_lastFrameIndex = index;
		return true;
	}

} // namespace bcd
