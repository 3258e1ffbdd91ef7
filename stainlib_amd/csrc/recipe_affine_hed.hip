// recipe_affine_hed.hip -- the one-pass recipe (recipe_kernels.hpp; launchers: recipe_launch.hpp): the affine view behind the HED stage, with and without the post stage.
// One of the translation units the recipe's kernel families are spread over, so that a parallel build compiles them side by side.
#include "recipe_launch.hpp"

template int sl::recipe_launch_affine<1, false>(const sl::RecipeCall&);
template int sl::recipe_launch_affine<1, true>(const sl::RecipeCall&);
