"""Host-side checks of the grouped deformable convolution's Python surface (no GPU): dcn_compat keeps the reference's divisibility error."""
import pytest


@pytest.mark.parametrize('C,K,group,dg', [(16, 8, 3, 1), (16, 6, 4, 1), (16, 8, 1, 3)])
def test_dcn_compat_divisibility_error_text(C, K, group, dg):
    import dualpixelface_amd.dcn_compat as DCN
    with pytest.raises(RuntimeError) as e:
        DCN._check_groups(C, K, group, dg)
    assert str(e.value) == 'channels(%d) and channels_out(%d) must divide group(%d) / deformable_group(%d)' % (C, K, group, dg)


@pytest.mark.parametrize('C,K,group,dg', [(16, 8, 1, 1), (16, 8, 2, 4), (16, 8, 4, 2), (12, 6, 3, 2), (8, 16, 8, 8)])
def test_dcn_compat_accepts_dividing_groupings(C, K, group, dg):
    import dualpixelface_amd.dcn_compat as DCN
    DCN._check_groups(C, K, group, dg)


def test_autograd_surface_has_the_grouping_keywords():
    import inspect
    from dualpixelface_amd import ops
    sig = inspect.signature(ops.deform_conv3d)
    assert sig.parameters['group'].default == 1 and sig.parameters['deformable_group'].default == 1
