// diasss_amd/host/frame.cpp -- Diasss::Frame over the C ABI (mirrors /root/reference/src/core/frame.cpp:18-55)
#include "frame.h"
#include "dsss_device.h"

namespace Diasss
{

bool Frame::USE_SIFT = false;

Frame::Frame(const int &id, const cv::Mat &mImg, const cv::Mat &mPose, const std::vector<double> &vAltt,
             const std::vector<double> &vGrange, const cv::Mat &mAnno)
{
    raw_img = mImg; dr_poses = mPose; altitudes = vAltt; ground_ranges = vGrange; img_id = id; anno_kps = mAnno;
    tf_stb = {0, 0, 0}; tf_port = {0, 0, 0};                                  // frame.cpp:38-39
    dsss_ctx* c = Device::ctx();
    // the waterfall goes down in the type it has (CV_8U, CV_16U, CV_32F or CV_64F): the library widens on the device, with the
    // results of the CV_64F image of the same samples
    const int raw_type = RawType(mImg);
    if (raw_type < 0) throw std::runtime_error("Frame: the waterfall must be CV_8U, CV_16U, CV_32F or CV_64F");
    Device::check(dsss_frame_set_typed(c, id, mImg.ptr<unsigned char>(), raw_type, mImg.rows, mImg.cols, mPose.ptr<double>(), vAltt.data(), vGrange.data()),
                  "dsss_frame_set_typed");
    geo_img = GetGeoImg(mImg.rows, mImg.cols, mPose, vGrange, tf_stb, tf_port);
    DetectFeature(norm_img, flt_mask, kps, dst);
}

int Frame::RawType(const cv::Mat &mImg)
{
    switch (mImg.type()) {
    case CV_64F: return DSSS_RAW_F64; case CV_32F: return DSSS_RAW_F32; case CV_16U: return DSSS_RAW_U16; case CV_8U: return DSSS_RAW_U8;
    default: return -1;
    }
}

void Frame::DetectFeature(const cv::Mat &, const cv::Mat &, std::vector<cv::KeyPoint> &out_kps, cv::Mat &out_dst)
{
    dsss_ctx* c = Device::ctx();
    int n = 0;
    dsss_orb_params op; dsss_orb_params_default(&op);                            // frame.cpp:180: ORBextractor(2000, 1.2, 6, 12, 7)
    op.descriptor = USE_SIFT ? DSSS_DESC_SIFT128 : DSSS_DESC_ORB;
    Device::check(dsss_set_params(c, nullptr, &op, nullptr, nullptr), "dsss_set_params");
    Device::check(dsss_extract(c, img_id, &n), "dsss_extract");
    std::vector<dsss_kp> k(n > 0 ? n : 1);
    if (USE_SIFT) {
        out_dst = cv::Mat(n, 128, CV_32F);
        Device::check(dsss_features_get(c, img_id, k.data(), nullptr, nullptr, n, &n), "dsss_features_get");
        Device::check(dsss_features_get_sift(c, img_id, n ? out_dst.ptr<float>() : nullptr, n, &n), "dsss_features_get_sift");
    } else {
        out_dst = cv::Mat(n, 32, CV_8U);
        Device::check(dsss_features_get(c, img_id, k.data(), n ? out_dst.data() : nullptr, nullptr, n, &n), "dsss_features_get");
    }
    out_kps.clear();
    for (int i = 0; i < n; ++i) out_kps.push_back(cv::KeyPoint(k[i].x, k[i].y, k[i].size, k[i].angle, k[i].response, k[i].octave));
}

std::vector<cv::Mat> Frame::GetGeoImg(const int &, const int &, const cv::Mat &, const std::vector<double> &,
                                      const std::vector<double> &, const std::vector<double> &)
{
    double bb[4];
    Device::check(dsss_frame_bbox(Device::ctx(), img_id, bb), "dsss_frame_bbox");
    cv::Mat gx(1, 2, CV_64F), gy(1, 2, CV_64F);
    gx.at<double>(0, 0) = bb[0]; gx.at<double>(0, 1) = bb[1]; gy.at<double>(0, 0) = bb[2]; gy.at<double>(0, 1) = bb[3];
    return { gx, gy };
}

void Frame::FetchImages()
{
    norm_img = cv::Mat(raw_img.rows, raw_img.cols, CV_8U); flt_mask = cv::Mat(raw_img.rows, raw_img.cols, CV_8U);
    Device::check(dsss_frame_get_norm(Device::ctx(), img_id, norm_img.data(), flt_mask.data()), "dsss_frame_get_norm");
}

void Frame::FetchGeoImg()
{
    cv::Mat gx(raw_img.rows, raw_img.cols, CV_64F), gy(raw_img.rows, raw_img.cols, CV_64F);
    Device::check(dsss_frame_get_geo(Device::ctx(), img_id, gx.ptr<double>(), gy.ptr<double>()), "dsss_frame_get_geo");
    geo_img = { gx, gy };
}

cv::Mat Frame::GetNormalizeSSS(const cv::Mat &) { if (norm_img.empty()) FetchImages(); return norm_img; }
cv::Mat Frame::GetFilteredMask(const cv::Mat &) { if (flt_mask.empty()) FetchImages(); return flt_mask; }

} // namespace Diasss
