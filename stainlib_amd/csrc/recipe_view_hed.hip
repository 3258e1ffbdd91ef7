// recipe_view_hed.hip -- the one-pass recipe (recipe_kernels.hpp; launchers: recipe_launch.hpp): the fixed-size and the resizing view behind the HED stage, with the post stage.
// One of the translation units the recipe's kernel families are spread over, so that a parallel build compiles them side by side.
#include "recipe_launch.hpp"

template int sl::recipe_launch_view<1>(const sl::RecipeCall&);
template int sl::recipe_launch_resize<1>(const sl::RecipeCall&);
